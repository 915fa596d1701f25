// The tiled tolerance-mode F kernels on the 64 x 8 tile: the LDS-read attribute, the tile geometry (XTileT, TTileT,
// FTile, FsTile, FSolve, fs_ring_cell), k_ftile (two sweeps per launch) and k_fsolve (a whole Chebyshev solve per
// launch) with their gates and launchers.  Declares the g1_* row helpers that mg_fused.inc defines.
// Needs mpbp.hip's prelude (KO, MPBP_HIP, set_error) and kernel sections: the epilogues, the F stencil (FStencilFast)
// and the marching kernels' sources (BNone, GxBT).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// ---- two F sweeps per launch on a 2D tile, tolerance mode (k_ftile) ----
// A workgroup owns a 64 x 8 tile of cells (two per lane: rows t>>6 and 4 + t>>6 of the tile, column t & 63).  It first
// stages, with coalesced loads, thn and (!INIT) x_in over the tile plus a two-cell halo (68 x 12 cells, 32.6 KB of LDS):
// every stencil operand after that is an LDS read at a constant offset from the cell's slot, with no periodic wrap and
// no 64-bit address arithmetic per neighbour.  Level A runs on the tile plus a one-cell halo (66 x 10 cells): INIT, the
// pointwise first iterate x0 = d0 = c2_0 b / diag (diag rebuilt from thn, FStencilFast::rdiag4); otherwise sweep s from
// x_in and d_in.  Level A's x replaces x_in in the same LDS slots (after a barrier: its stencil reads x_in around the
// cell), its d and the reciprocal diagonals of the lane's two tile cells stay in registers; level B (sweep 1, or s + 1)
// computes the tile from LDS, reusing those diagonals, and writes x_out (and d_out when SD).  Every workgroup is
// independent.  Each level performs the IEEE operations of the marching kernels' tolerance-mode rows and updates, so
// k_ftile is bit-identical to k_march_init + (k_march or) k_march2.  One GPU, whole grid.
// The LDS-tiled stencil kernels read each operand with its own ds_read_b64 (2 LDS cycles per wave on gfx950) instead
// of letting the compiler pair neighbouring slots into ds_read2_b64 (8 cycles: half the bytes per clock).
#ifndef MPBP_LDS_SINGLE
#define MPBP_LDS_SINGLE 1
#endif
#if MPBP_LDS_SINGLE && defined(__HIP_DEVICE_COMPILE__)   // (a device-code attribute: the host pass has no such feature)
#define MPBP_LDS_READS __attribute__((target("no-load-store-opt")))
#else
#define MPBP_LDS_READS
#endif
constexpr int kFTW = 64, kFTH = 8, kFSW = kFTW + 4, kFSH = kFTH + 4, kFSN = kFSW * kFSH;
template <int W, int H>
struct XTileT {  // 4 fields over a W x H block of LDS ([4][H][W]), slot (0, 0) = virtual grid cell (rb, cb)
    const double* x;
    int rb, cb;
    __device__ double X(int f, int r, int c) const { return x[(f * H + (r - rb)) * W + (c - cb)]; }
};
constexpr int kFAW = kFTW + 2, kFAH = kFTH + 2, kFAN = kFAW * kFAH;   // level A's cells: the tile + 1 halo
template <int W>
struct TTileT {  // staged thn at virtual grid coordinates, W columns per staged row
    const double* t;
    int rb, cb;
    __device__ double T(int sph, int r, int c) const {
        const double v = t[(r - rb) * W + (c - cb)];
        return sph ? 1.0 - v : v;
    }
};
template <int W>
struct TTileWT {  // staged thn at wrapped grid coordinates (GxBT::b: its wrap tests need the wrapped row / column)
    const double* t;
    int rb, cb, n;
    __device__ double T(int sph, int r, int c) const {
        int lr = r - rb, lc = c - cb;
        lr = lr < 0 ? lr + n : (lr >= n ? lr - n : lr);
        lc = lc < 0 ? lc + n : (lc >= n ? lc - n : lc);
        const double v = t[lr * W + lc];
        return sph ? 1.0 - v : v;
    }
};
struct FTile {
    const double* x_in;   // !INIT: x_{s-1}
    const double* d_in;   // !INIT: d_{s-1}
    const double* b;      // BNone: the right-hand side
    const double* sub;    // SUB: level B returns sub - x
    double* x_out;
    double* d_out;        // SD
    double c1a, c2a, c1b, c2b;   // INIT: c2a = c2_0 (c1a unused)
    int dzero = 0;        // !INIT: d_{s-1} is +0.0 (a restart: multigrid post-smoothing), d_in is not read
    const double* xc = nullptr;   // !INIT: x_in + P_0 xc (the coarse correction of a multigrid level 0, the F
                                  // hierarchy's MAC kinds) is the iterate -- the prolongation launch folded in
};

// multigrid level 1's tile and windows (k_gal1; the level-0 fused kernels stage the same windows)
constexpr int kG1W = 32, kG1H = 4;                          // coarse tile
constexpr int kG1FW = 2 * kG1W + 2, kG1FH = 2 * kG1H + 2;   // t1: fine [2 c0 - 1, 2 c0 + 2 W + 1)
constexpr int kG1PW = kG1FW + 2, kG1PH = kG1FH + 2;         // t0 and thn: one more fine cell each side
constexpr int kG1CW = kG1W + 4;                             // coarse x: [c0 - 2, c0 + W + 2)
template <int KY, int KX, int S = kG1CW>
__device__ inline double g1_p(const double* xf, int gr, int gc, int nc, int rb, int cb);
template <int KY, int KX, int S = kG1CW>
__device__ inline double g1_p_in(const double* xf, int r, int c);
template <int KY, int KX, int W, int OFF>
__device__ inline double g1_rw_in(const double* tf, int lr, int lc);
__device__ inline bool g1_inner(int cr0, int cc0, int th, int tw, int nc);
template <bool INIT, bool SUB, bool SD, class BS, bool PRO = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) MPBP_LDS_READS k_ftile(FStencilFast P, FTile a, BS bs) {
    __shared__ double xs[INIT ? 1 : 4 * kFSN];   // !INIT: x_in over the tile + 2 halo
    __shared__ double ts[kFSN];                   // thn over the tile + 2 halo
    __shared__ double xl[4 * kFAN];               // level A's x over the tile + 1 halo (PRO: first the coarse window)
    const int n = P.n;
    const int tx = (n + kFTW - 1) / kFTW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int r0 = (bk / tx) * kFTH, c0 = (bk % tx) * kFTW;
    const int rb = r0 - 2, cb = c0 - 2;
    const int tid = threadIdx.x;
    const int nn = n * n;
    // PRO: the coarse correction over [r0 / 2 - 2, r0 / 2 + 6) x [c0 / 2 - 2, c0 / 2 + 34) of 4 fields (k_gal1's window)
    constexpr int CW = kFTW / 2 + 4, CH = kFTH / 2 + 4, CN = CW * CH;
    static_assert(!PRO || 4 * CN <= 4 * kFAN, "the coarse window fits the level-A buffer");
    static_assert(CW == kG1CW && kFSW == kG1PW && kFSH == kG1PH, "g1_p_in's window geometry");
    const int nc = n >> 1, ncc = nc * nc, cr0 = r0 >> 1, cc0 = c0 >> 1;
    // stage thn (and x_in) over rows r0-2 .. r0+9, columns c0-2 .. c0+65: every load issued before the first LDS store
    {
        constexpr int IT = (kFSN + 255) / 256, NF = INIT ? 1 : 5, IC = PRO ? (4 * CN + 255) / 256 : 1;
        double v[IT][NF], vc[IC];
        if constexpr (PRO) {
            auto wrapc = [&](int q) { return q < 0 ? q + nc : (q >= nc ? q - nc : q); };
#pragma unroll
            for (int it = 0; it < IC; ++it) {
                const int i = tid + it * 256;
                if (i < 4 * CN) {
                    const int f = i / CN, j = i - f * CN, r = j / CW, c = j - r * CW;
                    vc[it] = a.xc[f * ncc + wrapc(cr0 - 2 + r) * nc + wrapc(cc0 - 2 + c)];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < kFSN) {
                const int sr = i / kFSW, sc = i - sr * kFSW;
                const int32_t k = P.wrap(rb + sr) * n + P.wrap(cb + sc);
                v[it][0] = P.cell[k];
                if constexpr (!INIT) {
#pragma unroll
                    for (int f = 0; f < 4; ++f) v[it][1 + f] = a.x_in[f * nn + k];
                }
            }
        }
        if constexpr (PRO) {
#pragma unroll
            for (int it = 0; it < IC; ++it)
                if (tid + it * 256 < 4 * CN) xl[tid + it * 256] = vc[it];
            __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < kFSN) {
                ts[i] = v[it][0];
                if constexpr (!INIT) {
                    if constexpr (PRO) {   // x_in + P_0 xc: k_mg_transfer_spmv's prolongation and EpiAdd's sum
                        const int sr = i / kFSW, sc = i - sr * kFSW;
                        const int gr = P.wrap(rb + sr), gc = P.wrap(cb + sc);
                        const bool inner = g1_inner(cr0, cc0, kFTH / 2, kFTW / 2, nc);   // (window coordinates)
#pragma unroll
                        for (int f = 0; f < 4; ++f) {
                            const double pc =
                                inner ? ((f & 1) ? g1_p_in<MPBP_MG_NODE, MPBP_MG_CELL>(xl + f * CN, sr, sc)
                                                 : g1_p_in<MPBP_MG_CELL, MPBP_MG_NODE>(xl + f * CN, sr, sc))
                                      : ((f & 1) ? g1_p<MPBP_MG_NODE, MPBP_MG_CELL>(xl + f * CN, gr, gc, nc, cr0 - 2, cc0 - 2)
                                                 : g1_p<MPBP_MG_CELL, MPBP_MG_NODE>(xl + f * CN, gr, gc, nc, cr0 - 2, cc0 - 2));
                            xs[f * kFSN + i] = pc + v[it][1 + f];
                        }
                    } else {
#pragma unroll
                        for (int f = 0; f < 4; ++f) xs[f * kFSN + i] = v[it][1 + f];
                    }
                }
            }
        }
    }
    __syncthreads();
    const TTileT<kFSW> tt{ts, rb, cb};
    const TTileWT<kFSW> tw{ts, rb, cb, n};
    const XTileT<kFSW, kFSH> xa{xs, rb, cb};
    const XTileT<kFAW, kFAH> xb{xl, rb + 1, cb + 1};
    // level A at virtual cell (vr, vc): its x (xn), d (dA) and the reciprocal diagonals (rd)
    auto level_a = [&](int vr, int vc, double* dA, double* rd) {
        const int si = (vr - rb - 1) * kFAW + (vc - cb - 1);
        const int gr = P.wrap(vr), gc = P.wrap(vc);
        const int32_t k = gr * n + gc;
        double bv[4];
        typename BS::Q q{};
        if constexpr (BS::on) q = bs.load(gr, gr, gc);
        else {
#pragma unroll
            for (int f = 0; f < 4; ++f) bv[f] = a.b[f * nn + k];
        }
        const FStencilDev::Stage sg{{P.uface[k], P.vface[k]}};
        if constexpr (INIT) {
            P.rdiag4(vr, vc, tt, sg, rd);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double bf = BS::on ? bs.b(f, gr, gc, gc, tw, q) : bv[f];
                const double x0 = a.c2a * bf * rd[f];
                xl[f * kFAN + si] = x0;
                dA[f] = x0;
            }
        } else {
            double acc[4];
            P.rows4(vr, vc, tt, xa, FStencilDev::Cell{{sg.face[0], sg.face[1]}}, acc, rd);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double bf = BS::on ? bs.b(f, gr, gc, gc, tw, q) : bv[f];
                const double z = (bf - acc[f]) * rd[f];
                const double dprev = a.dzero ? 0.0 : a.d_in[f * nn + k];
                const double dn = a.c1a * dprev + a.c2a * z;
                xl[f * kFAN + si] = xa.X(f, vr, vc) + dn;
                dA[f] = dn;
            }
        }
    };
    const int lc = tid & 63, lr = tid >> 6;
    double dA0[4], dA1[4], rd0[4], rd1[4];
    level_a(r0 + lr, c0 + lc, dA0, rd0);
    level_a(r0 + 4 + lr, c0 + lc, dA1, rd1);
    // the halo ring: rows -1 and kFTH (66 cells each), columns -1 and kFTW of rows 0 .. kFTH-1: 148 cells
    constexpr int kRing = 2 * (kFTW + 2) + 2 * kFTH;
    if (tid < kRing) {
        int hr, hc;
        if (tid < 2 * (kFTW + 2)) {
            const int j = tid < kFTW + 2 ? tid : tid - (kFTW + 2);
            hr = tid < kFTW + 2 ? r0 - 1 : r0 + kFTH;
            hc = c0 - 1 + j;
        } else {
            const int j = tid - 2 * (kFTW + 2);
            hr = r0 + (j >> 1);
            hc = (j & 1) ? c0 + kFTW : c0 - 1;
        }
        double dh[4], rh[4];
        level_a(hr, hc, dh, rh);
    }
    __syncthreads();
    // level B on the tile's own cells
    auto level_b = [&](int vr, int vc, const double* dA, const double* rdA) {
        if (vr >= n || vc >= n) return;   // a tile past the grid's last row / column
        const int32_t k = vr * n + vc;
        const FStencilDev::Cell cl{{P.uface[k], P.vface[k]}};
        double acc[4], rdx[4];
        P.template rows4<false>(vr, vc, tt, xb, cl, acc, rdx);
        typename BS::Q q{};
        if constexpr (BS::on) q = bs.load(vr, vr, vc);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double bf = BS::on ? bs.b(f, vr, vc, vc, tw, q) : a.b[f * nn + k];
            const double z = (bf - acc[f]) * rdA[f];
            const double dn = a.c1b * dA[f] + a.c2b * z;
            const int32_t o = f * nn + k;
            if constexpr (SD) a.d_out[o] = dn;
            const double x = xb.X(f, vr, vc) + dn;
            a.x_out[o] = SUB ? a.sub[o] - x : x;
        }
    };
    level_b(r0 + lr, c0 + lc, dA0, rd0);
    level_b(r0 + 4 + lr, c0 + lc, dA1, rd1);
}

template <bool INIT, bool SUB, bool SD, class BS>
int launch_ftile_t(const FStencilFast& P, const FTile& a, hipStream_t st, const BS& bs) {
    const int64_t tiles = (int64_t)((P.n + kFTW - 1) / kFTW) * ((P.n + kFTH - 1) / kFTH);
    if constexpr (!INIT && !BS::on) {
        if (a.xc) {
            k_ftile<INIT, SUB, SD, BS, true><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
            MPBP_HIP(hipGetLastError());
            return MPBP_OK;
        }
    }
    k_ftile<INIT, SUB, SD, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
// INIT: level A = x0, level B = sweep 1 (the solve's first two updates); else sweeps s, s + 1.  One GPU, whole grid.
// Grids whose cells a tile and its staged halo wrap onto at most once each way.
inline bool ftile_ok(int n) { return n >= kFTW + kFTH + 4; }
template <bool INIT, class BS = BNone>
int launch_ftile(const FStencilDev& Pd, const FTile& a, hipStream_t st, const BS& bs = BS{}) {
    const FStencilFast P{Pd};
    if (P.h != 0 || P.which != 0 || !ftile_ok(P.n)) return set_error(MPBP_ERR_ARG, "ftile: one GPU, whole grid, n >= 76");
    if (!a.x_out || (!INIT && (!a.x_in || (!a.d_in && !a.dzero) || a.x_in == a.x_out)) || (!BS::on && !a.b) ||
        (a.d_out && (a.d_out == a.d_in || a.d_out == a.x_in)) || (a.xc && (INIT || BS::on || (P.n & 1))))
        return set_error(MPBP_ERR_ARG, "ftile: bad vectors");
    const bool sub = a.sub != nullptr, sd = a.d_out != nullptr;
    return sub ? (sd ? launch_ftile_t<INIT, true, true>(P, a, st, bs) : launch_ftile_t<INIT, true, false>(P, a, st, bs))
               : (sd ? launch_ftile_t<INIT, false, true>(P, a, st, bs) : launch_ftile_t<INIT, false, false>(P, a, st, bs));
}

// ---- a whole tolerance-mode F Chebyshev solve in one launch (k_fsolve) ----
// x = F^-1 b by K = H + 1 Chebyshev-Jacobi updates from x0 = 0 (the first is the pointwise x0 = d0 = c2_0 b / diag),
// on the 64 x 8 tiles of k_ftile: thn is staged over the tile plus H + 1 halo cells, level 0 builds x0 over the tile
// plus H, and level l = 1 .. H recomputes the tile plus H - l from level l - 1 (LDS ping-pong), the last writing x.
// Every cell a workgroup computes has one owning lane for all its levels: the lane's two tile cells (as k_ftile) and
// cell t of each halo ring r = 1 .. H (140 + 8 r cells, lane t < that), so its d, b, faces and reciprocal diagonals
// stay in that lane's registers from level 0 on.  Each level performs the IEEE operations of the marching kernels'
// tolerance-mode rows and updates: bit-identical to k_ftile<INIT> + k_ftile pair (H = 3) or + k_ftile sweep.  HBM:
// b (or x_p), thn, faces in, x out once -- against x, d, b re-read per launch by the two-launch solve.
template <int H>
struct FsTile {
    static constexpr int RW = kFTW + 2 * H, RH = kFTH + 2 * H, N = RW * RH;   // x levels: the tile + H
    static constexpr int TW = RW + 2, TH = RH + 2, TN = TW * TH;             // thn: the tile + H + 1
};
struct FSolve {
    const double* b;      // BNone: the right-hand side
    const double* sub;    // the result is sub - x when set
    double* x_out;
    double c2_0;
    double c1[4], c2[4];  // updates 1 .. H
};
// ring r's cell j: rows r0 - r and r0 + TH - 1 + r (all 64 + 2r columns), then columns c0 - r and c0 + TW - 1 + r of
// the rows between
__device__ inline void fs_ring_cell(int r, int j, int r0, int c0, int& vr, int& vc) {
    const int w = kFTW + 2 * r;
    if (j < 2 * w) {
        vr = j < w ? r0 - r : r0 + kFTH - 1 + r;
        vc = c0 - r + (j < w ? j : j - w);
    } else {
        const int k = j - 2 * w;
        vr = r0 - r + 1 + (k >> 1);
        vc = (k & 1) ? c0 + kFTW - 1 + r : c0 - r;
    }
}

// PART (row partition, the CA schedule): the tiles cover the owned rows and P.ext ghost rows each side; b and x are
// in the partition's ghost layout (P.xrow, P.out_row), the thn tables global.  Rows past b's ghost depth (padding of
// the last tile row and its halo, which no output reads) load a clamped row.
template <int H, bool SUB, bool PART, class BS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) MPBP_LDS_READS
k_fsolve(FStencilFast P, FSolve a, BS bs) {
    using T = FsTile<H>;
    constexpr int NT = 2;       // tile cells per lane
    constexpr int NSL = H + 2;  // owned cells per lane: the tile's two (rows lr, lr + 4), then ring r at slot 1 + r
    constexpr int NS = H + 1;   // ... with updates after x0 (ring H only needs x0)
    constexpr int PW = T::RW + 1, PN = PW * (T::RH + 1);   // BS: x_p over the tile + H, + its west / north neighbours
    __shared__ double ts[T::TN];
    __shared__ double xa[4 * T::N], xb[4 * T::N];
    __shared__ double ps[BS::on ? PN : 1];
    const int n = P.n, nn = n * n;
    const int tx = (n + kFTW - 1) / kFTW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int lo = PART ? P.r0 - P.ext : 0, hi = PART ? P.r0 + P.L + P.ext : n;   // output rows [lo, hi)
    const int r0 = lo + (bk / tx) * kFTH, c0 = (bk % tx) * kFTW;
    const int rbt = r0 - H - 1, cbt = c0 - H - 1, rb = r0 - H, cb = c0 - H;
    const int tid = threadIdx.x;
    // a row of the input layouts: the virtual row itself (one GPU: wrapped) or, clamped to the ghost depth, local
    auto in_row = [&](int vr, int h) {
        if constexpr (PART) {
            const int lr = vr - P.r0;
            return lr < -h ? -h : (lr >= P.L + h ? P.L + h - 1 : lr);
        } else {
            return P.wrap(vr);
        }
    };
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
    if constexpr (BS::on) {
        constexpr int IT = (PN + 255) / 256;
        double v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < PN) {
                const int sr = i / PW, sc = i - sr * PW;
                const int pr = in_row(rb - 1 + sr, PART ? bs.h : 0);
                v[it] = bs.xp[(PART ? ext_row(1, 0, pr, P.L, bs.h, n) : pr * n) + P.wrap(cb - 1 + sc)];
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < PN) ps[i] = v[it];
        }
    }
    const int lr = tid >> 6, lc = tid & 63;
    // the owned cells and their rings (0: a tile cell; ring r lives through level H - r)
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
    // every owned cell's faces and b (BNone) are loaded here, behind the staging loads and ahead of the barrier: one
    // global-memory latency for the whole level 0 instead of one per cell
    constexpr bool LB = !BS::on || BS::resid;   // b (BNone) or z (GxR) loaded per owned cell
    static_assert(!(BS::resid && (PART || SUB)), "GxR: one GPU, no sub");
    double fl[NSL][2], bl[LB ? NSL : 1][4];
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own[sl]) continue;
        const int gr = P.wrap(cr[sl]), gc = P.wrap(cc[sl]);
        const int32_t k = gr * n + gc;
        fl[sl][0] = P.uface[k];
        fl[sl][1] = P.vface[k];
        if constexpr (BS::resid) {
#pragma unroll
            for (int f = 0; f < 4; ++f) bl[sl][f] = bs.z[(f * n + gr) * n + gc];
        } else if constexpr (!BS::on) {
            const int br = in_row(cr[sl], P.h);
#pragma unroll
            for (int f = 0; f < 4; ++f) bl[sl][f] = a.b[(PART ? ext_row(4, f, br, P.L, P.h, n) : (f * n + br) * n) + gc];
        }
    }
    __syncthreads();
    const TTileT<T::TW> tt{ts, rbt, cbt};
    double d[NS][4], rd[NS][4], bv[NS][4], fc[NS][2];
    // level 0: x0 = d0 = c2_0 b / diag over the tile + H
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own[sl]) continue;
        const int vr = cr[sl], vc = cc[sl];
        const int gr = P.wrap(vr), gc = P.wrap(vc);
        const FStencilDev::Stage sg{{fl[sl][0], fl[sl][1]}};
        double b4[4], r4[4];
        P.rdiag4(vr, vc, tt, sg, r4);
        if constexpr (BS::on) {   // b = G x_p, x_p and thn from LDS at virtual coordinates
            const int pi = (vr - rb + 1) * PW + (vc - cb + 1);
            const typename BS::Q q{ps[pi], ps[pi - 1], ps[pi - PW]};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                b4[f] = bs.b_at(f, vr, vc, gc == 0, gr == 0, tt, q);
                if constexpr (BS::resid) b4[f] = bl[sl][f] - b4[f];   // z - (G x_p), EpiResid's subtraction
            }
        } else {
#pragma unroll
            for (int f = 0; f < 4; ++f) b4[f] = bl[sl][f];
        }
        const int si = (vr - rb) * T::RW + (vc - cb);
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
            fc[sl][0] = sg.face[0];
            fc[sl][1] = sg.face[1];
        }
    }
    // levels 1 .. H
    double* cur = xa;
    double* nxt = xb;
    double sv[NT][4];   // SUB: the tile cells' sub entries, loaded at the start of level H (its stencil work hides them)
#pragma unroll
    for (int l = 1; l <= H; ++l) {
        __syncthreads();
        const XTileT<T::RW, T::RH> xt{cur, rb, cb};
        const double c1 = a.c1[l - 1], c2 = a.c2[l - 1];
        if constexpr (SUB) {
            if (l == H) {
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    const int vr = cr[m], vc = cc[m];
                    if (vr >= hi || vc >= n) continue;
#pragma unroll
                    for (int f = 0; f < 4; ++f)
                        sv[m][f] = a.sub[PART ? P.out_row(f, vr - P.r0, vc) : f * nn + vr * n + vc];
                }
            }
        }
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            if (sl >= NT && (!own[sl] || rr[sl] > H - l)) continue;   // ring r lives through level H - r
            const int vr = cr[sl], vc = cc[sl];
            if (l == H && (vr >= hi || vc >= n)) continue;            // a tile past the last row / column
            double acc[4], rdx[4];
            P.template rows4<false>(vr, vc, tt, xt, FStencilDev::Cell{{fc[sl][0], fc[sl][1]}}, acc, rdx);
            const int si = (vr - rb) * T::RW + (vc - cb);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double z = (bv[sl][f] - acc[f]) * rd[sl][f];
                const double dn = c1 * d[sl][f] + c2 * z;
                const double x = cur[f * T::N + si] + dn;
                if (l < H) {
                    nxt[f * T::N + si] = x;
                    d[sl][f] = dn;
                } else {
                    const int32_t o = PART ? P.out_row(f, vr - P.r0, vc) : f * nn + vr * n + vc;
                    if constexpr (SUB) a.x_out[o] = sv[sl < NT ? sl : 0][f] - x;   // (level H: tile cells only)
                    else a.x_out[o] = x;
                }
            }
        }
        double* t = cur;
        cur = nxt;
        nxt = t;
    }
}

// Grids a tile's staged thn (tile + H + 1 each side) wraps onto at most once.
template <int H>
inline bool fsolve_ok_n(int n) { return n >= FsTile<H>::TW && n >= FsTile<H>::TH; }
template <int H, bool PART, class BS>
int launch_fsolve_t(const FStencilFast& P, const FSolve& a, hipStream_t st, const BS& bs) {
    const int rows = PART ? P.L + 2 * P.ext : P.n;
    const int64_t tiles = (int64_t)((P.n + kFTW - 1) / kFTW) * ((rows + kFTH - 1) / kFTH);
    if constexpr (BS::resid) {   // GxR: the upper block form's solve, never subtracted from anything
        if (a.sub) return set_error(MPBP_ERR_ARG, "fsolve: the z - G x_p right-hand side takes no sub");
        k_fsolve<H, false, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    } else {
    if (a.sub) k_fsolve<H, true, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    else k_fsolve<H, false, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    }
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

}  // namespace
