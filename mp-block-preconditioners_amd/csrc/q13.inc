// Gt_F_G on the 13-point diamond: the diamond-layout kernels, k_qmf (matrix-free, tolerance mode) and the svl / q13
// C ABI.  Needs mpbp.hip's Csr, epilogues and FStencilFast, XTileT / TTileT (f_tile.inc), PGDev (pg_stencil.inc),
// svl_spmv / svl_cheb (launchers.inc) and abi_stencil.inc (make_fstencil, make_pgstencil).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

// ================================================ Gt_F_G, 13-point diamond ====
// Gt_F_G = ((-D) F) G couples every pressure cell with the 13 cells of the diamond |dr| + |dc| <= 2 (n >= 5;
// every structural product kept, so every row has exactly these 13 entries).  The diamond layout stores the
// values alone, slot-major (vals[s * N + cell], slots in (dr, dc) lexicographic order = the CSR row's column
// order for a cell whose diamond does not wrap), and rebuilds the columns from the grid: 104 B per row
// instead of SELL's 156 B of values + column indices.  A cell within two rows / columns of the periodic edge
// has its columns in wrapped order; its wave sorts the 13 products by wrapped column (a transposition
// network in registers) and sums them in that order -- the CSR SpMV's additions exactly, bit for bit.
// Rebuilding the values themselves from thn (as the D / G / Gt_G sweeps do) would cost ~1000 fp64
// operations per row (8 F rows of 10 entries, 80 + 96 products, first-touch accumulation): on this chip that
// is slower than streaming the 104 B.
namespace {
constexpr int kQSlots = 13;
__device__ __host__ constexpr int q13_dr(int s) { return s < 1 ? -2 : s < 4 ? -1 : s < 9 ? 0 : s < 12 ? 1 : 2; }
__device__ __host__ constexpr int q13_dc(int s) {
    return s < 1 ? 0 : s < 4 ? s - 2 : s < 9 ? s - 6 : s < 12 ? s - 10 : 0;
}
// slot of offset (dr, dc), or -1 outside the diamond
__device__ inline int q13_slot(int dr, int dc) {
    const int a = (dr < 0 ? -dr : dr) + (dc < 0 ? -dc : dc);
    if (a > 2) return -1;
    return dr == -2 ? 0 : dr == -1 ? 2 + dc : dr == 0 ? 6 + dc : dr == 1 ? 10 + dc : 12;
}
__device__ inline int q13_off(int d, int n) {   // periodic offset folded into [-2, 2], or 99
    if (d > 2) d -= n;
    if (d < -2) d += n;
    return (d >= -2 && d <= 2) ? d : 99;
}

// row0 (a row partition's block, mpbp_q13_build_rows): Q's row r is grid row (row0 + r / n) mod n, column r % n;
// vals holds Q->nrows cells per slot
__global__ void k_q13_fill(Csr Q, int32_t N, int32_t n, double* vals, int* bad, int32_t row0 = 0) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    int gr = row0 + r / n;
    gr = ((gr % n) + n) % n;
    const int gc = r - (r / n) * n;
    unsigned seen = 0;
    bool ok = Q.rp[r + 1] - Q.rp[r] == kQSlots;
    for (int32_t k = Q.rp[r]; ok && k < Q.rp[r + 1]; ++k) {
        const int32_t j = Q.ci[k];
        const int s = q13_slot(q13_off(j / n - gr, n), q13_off(j - (j / n) * n - gc, n));
        if (s < 0 || ((seen >> s) & 1u)) {
            ok = false;
            break;
        }
        seen |= 1u << s;
        vals[(int64_t)s * N + r] = Q.va[k];
    }
    if (!ok) atomicAdd(bad, 1);
}

// SYM (tolerance mode): Gt_F_G = G^T F G is symmetric, so its values are read from the upper half of the diamond
// alone -- slots 6 .. 12 ((0, 0) .. (2, 0)) at the cell, and slot 12 - s at the cell's neighbour (dr_s, dc_s) for the
// lower slots s = 0 .. 5, Q(c, c + o) = Q(c + o, c) -- 56 instead of 104 B of values per row (the mirrored reads are the
// neighbouring rows' own, cached).  The stored product is symmetric to rounding (|Q - Q^T| ~ 1.5e-16 |Q|): within the
// tolerance mode's bar, not bit-exact.
template <class Epi, bool SYM = false>
__global__ void __launch_bounds__(kBlock) k_q13(int32_t n, const double* __restrict__ vals,
                                                const double* __restrict__ x, Epi epi) {
    const int32_t N = n * n;
    const int32_t cell = xcd_swizzle(blockIdx.x, gridDim.x) * kBlock + threadIdx.x;
    if (cell >= N) return;
    const typename Epi::P pe = epi.pre(cell);
    const int gr = cell / n, gc = cell - (cell / n) * n;
    double v[kQSlots];
    const bool wraps = gr < 2 || gr >= n - 2 || gc < 2 || gc >= n - 2;
    if constexpr (SYM) {
#pragma unroll
        for (int s = 6; s < kQSlots; ++s) v[s] = vals[(int64_t)s * N + cell];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            int rr = gr + q13_dr(s), cc = gc + q13_dc(s);
            rr = rr < 0 ? rr + n : rr >= n ? rr - n : rr;
            cc = cc < 0 ? cc + n : cc >= n ? cc - n : cc;
            v[s] = vals[(int64_t)(12 - s) * N + rr * n + cc];
        }
    } else {
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) v[s] = __builtin_nontemporal_load(vals + (int64_t)s * N + cell);
    }
    double acc = 0.0;
    if (!__any(wraps)) {
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) acc += v[s] * x[cell + q13_dr(s) * n + q13_dc(s)];
    } else {   // (wrapped column, product) pairs sorted by column, then summed in that order
        int32_t key[kQSlots];
        double pr[kQSlots];
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) {
            int rr = gr + q13_dr(s), cc = gc + q13_dc(s);
            rr = rr < 0 ? rr + n : rr >= n ? rr - n : rr;
            cc = cc < 0 ? cc + n : cc >= n ? cc - n : cc;
            key[s] = rr * n + cc;
            pr[s] = v[s] * x[key[s]];
        }
#pragma unroll
        for (int round = 0; round < kQSlots; ++round) {
#pragma unroll
            for (int i = round & 1; i + 1 < kQSlots; i += 2) {
                const bool sw = key[i] > key[i + 1];
                const int32_t ka = key[i], kb = key[i + 1];
                const double pa = pr[i], pb = pr[i + 1];
                key[i] = sw ? kb : ka;
                key[i + 1] = sw ? ka : kb;
                pr[i] = sw ? pb : pa;
                pr[i + 1] = sw ? pa : pb;
            }
        }
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) acc += pr[s];
    }
    epi(cell, acc, pe);
}

// The symmetric-half read on a row partition (the owned grid rows [r0, r0 + L) of every rank): vals holds the diamond
// of grid rows r0 - 2 .. r0 + L - 1 (L + 2 rows: the lower slots of the first owned rows come from the two rows above),
// x the owned rows with h >= 2 ghost rows each side (ext_row layout).  Every value, product and the order of the sum
// (slot order, or for cells whose diamond wraps the periodic edge the wrapped global column order) are k_q13<SYM>'s:
// the rank's rows of the one-GPU result bit for bit.
template <class Epi>
__global__ void __launch_bounds__(kBlock) k_q13p(int32_t n, int32_t r0, int32_t L, int32_t h,
                                                 const double* __restrict__ vals, const double* __restrict__ x, Epi epi) {
    const int32_t M = (L + 2) * n;   // cells per slot of the row block
    const int32_t cell = xcd_swizzle(blockIdx.x, gridDim.x) * kBlock + threadIdx.x;
    if (cell >= L * n) return;
    const typename Epi::P pe = epi.pre(cell);
    const int lr = cell / n, gc = cell - (cell / n) * n, gr = r0 + lr;
    const int32_t bc = (lr + 2) * n + gc;   // the cell in the row block
    auto wrapc = [&](int c) { return c < 0 ? c + n : c >= n ? c - n : c; };
    double v[kQSlots];
#pragma unroll
    for (int s = 6; s < kQSlots; ++s) v[s] = vals[(int64_t)s * M + bc];
#pragma unroll
    for (int s = 0; s < 6; ++s) v[s] = vals[(int64_t)(12 - s) * M + (lr + 2 + q13_dr(s)) * n + wrapc(gc + q13_dc(s))];
    double pr[kQSlots];
    int32_t key[kQSlots];
#pragma unroll
    for (int s = 0; s < kQSlots; ++s) {
        const int cc = wrapc(gc + q13_dc(s));
        int rr = gr + q13_dr(s);
        rr = rr < 0 ? rr + n : rr >= n ? rr - n : rr;
        key[s] = rr * n + cc;
        pr[s] = v[s] * x[ext_row(1, 0, lr + q13_dr(s), L, h, n) + cc];
    }
    double acc = 0.0;
    const bool wraps = gr < 2 || gr >= n - 2 || gc < 2 || gc >= n - 2;
    if (!__any(wraps)) {
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) acc += pr[s];
    } else {
#pragma unroll
        for (int round = 0; round < kQSlots; ++round) {
#pragma unroll
            for (int i = round & 1; i + 1 < kQSlots; i += 2) {
                const bool sw = key[i] > key[i + 1];
                const int32_t ka = key[i], kb = key[i + 1];
                const double pa = pr[i], pb = pr[i + 1];
                key[i] = sw ? kb : ka;
                key[i + 1] = sw ? ka : kb;
                pr[i] = sw ? pb : pa;
                pr[i + 1] = sw ? pa : pb;
            }
        }
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) acc += pr[s];
    }
    epi(cell, acc, pe);
}

// max |Q(c, c + o) - Q(c + o, c)| over the diamond (slot s at c against slot 12 - s at c + o) and max |Q|: whether the
// symmetric-half read (k_q13<SYM>) may stand in for the stored product.  Non-negative doubles order like their bits.
__global__ void __launch_bounds__(kBlock) k_q13_asym(int32_t n, const double* __restrict__ vals,
                                                     unsigned long long* out) {
    const int32_t N = n * n;
    const int32_t cell = blockIdx.x * kBlock + threadIdx.x;
    double asym = 0.0, amax = 0.0;
    if (cell < N) {
        const int gr = cell / n, gc = cell - (cell / n) * n;
#pragma unroll
        for (int s = 0; s < kQSlots; ++s) amax = fmax(amax, fabs(vals[(int64_t)s * N + cell]));
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            int rr = gr + q13_dr(s), cc = gc + q13_dc(s);
            rr = rr < 0 ? rr + n : rr >= n ? rr - n : rr;
            cc = cc < 0 ? cc + n : cc >= n ? cc - n : cc;
            asym = fmax(asym, fabs(vals[(int64_t)s * N + cell] - vals[(int64_t)(12 - s) * N + rr * n + cc]));
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        asym = fmax(asym, __shfl_xor(asym, o));
        amax = fmax(amax, __shfl_xor(amax, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(out, (unsigned long long)__double_as_longlong(asym));
        atomicMax(out + 1, (unsigned long long)__double_as_longlong(amax));
    }
}

template <class Epi>
int launch_q13(int32_t n, const double* vals, const double* x, Epi epi, hipStream_t st, bool sym = false) {
    if (sym) k_q13<Epi, true><<<grid_for((int64_t)n * n), kBlock, 0, st>>>(n, vals, x, epi);
    else k_q13<Epi, false><<<grid_for((int64_t)n * n), kBlock, 0, st>>>(n, vals, x, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// ---- x_b = Gt_F_G x_a matrix-free, tolerance mode (k_qmf, kernel option q13_mf) ----
// solve.py:247-249 forms Gt_F_G = ((-D) F) G once and the apply multiplies it (k_q13: 7 or 13 stored diamond values
// per row, 75-126 MB per apply at 1024^2).  Here the product is applied as its three factors on a 32 x 16 tile of
// pressure cells: y = G x_a on the tile + 1 (its four velocity rows, GxBT::b_at's entries: d_p (+-inv g) with g the
// face's thn average), z = F y on the tile's cells plus their east / south faces (the tolerance-mode rows,
// FStencilFast::rows4_co), then x_b = -(D z) (DStencilDev's entries: +-inv times the face average).  x_a and thn are
// staged over the tile + 2, y and z live in LDS (z over y), only the faces of the z cells and x_b touch memory
// besides: HBM 8 B x_a + 24 B thn / faces + 8 B x_b per cell = 42 MB at 1024^2, against k_q13<SYM>'s 76 MB.  The same
// operator as the stored product; its sums in another order (a few ulp per entry, within north_star's 1e-12 on the
// apply: tests/test_gpu_fast.py, test_gpu_q13.py).  One GPU, whole grid, fast numerics, matrix-free F / D / G.
constexpr int kQmW = 32, kQmH = 16;
constexpr int kQxW = kQmW + 4, kQxH = kQmH + 4, kQxN = kQxW * kQxH;   // x_a, thn: the tile + 2
constexpr int kQyW = kQmW + 3, kQyH = kQmH + 3, kQyN = kQyW * kQyH;   // y = G x_a: rows / columns -1 .. +TW+1
constexpr int kQzW = kQmW + 1, kQzH = kQmH + 1, kQzN = kQzW * kQzH;   // z = F y: the tile's cells + east / south
template <class Epi>
__global__ void __launch_bounds__(256) MPBP_LDS_READS k_qmf(FStencilFast P, PGDev G, const double* __restrict__ xa,
                                                            Epi epi) {
    __shared__ double ts[kQxN], xs[kQxN];
    __shared__ double ys[4 * kQyN];   // y; then z (4 * kQzN <= 4 * kQyN)
    const int n = P.n;
    const int tx = (n + kQmW - 1) / kQmW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int r0 = (bk / tx) * kQmH, c0 = (bk % tx) * kQmW;
    const int tid = threadIdx.x;
    constexpr int IX = (kQxN + 255) / 256, IZ = (kQzN + 255) / 256;
    {   // x_a and thn over the tile + 2; the faces of this lane's z cells -- every load before the first LDS store
        double vt[IX], vx[IX];
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i < kQxN) {
                const int sr = i / kQxW, sc = i - sr * kQxW;
                const int32_t k = P.wrap(r0 - 2 + sr) * n + P.wrap(c0 - 2 + sc);
                vt[it] = P.cell[k];
                vx[it] = xa[k];
            }
        }
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i < kQxN) {
                ts[i] = vt[it];
                xs[i] = vx[it];
            }
        }
    }
    double fu[IZ], fv[IZ];
#pragma unroll
    for (int it = 0; it < IZ; ++it) {
        const int i = tid + it * 256;
        if (i < kQzN) {
            const int zr = i / kQzW, zc = i - zr * kQzW;
            const int32_t k = P.wrap(r0 + zr) * n + P.wrap(c0 + zc);
            fu[it] = P.uface[k];
            fv[it] = P.vface[k];
        }
    }
    __syncthreads();
    const TTileT<kQxW> tt{ts, r0 - 2, c0 - 2};
    const XTileT<kQxW, 1> xt{xs, r0 - 2, c0 - 2};
    // y = G x_a: velocity rows (u_n, v_n, u_s, v_s) at (r, c) -- u on the cell's west face, v on its north face
    for (int i = tid; i < kQyN; i += 256) {
        const int vr = r0 - 1 + i / kQyW, vc = c0 - 1 + i % kQyW;
        const double xc = xt.X(0, vr, vc), xw = xt.X(0, vr, vc - 1), xn = xt.X(0, vr - 1, vc);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double t0 = tt.T(p, vr, vc);
            const double gu = 0.5 * (t0 + tt.T(p, vr, vc - 1)), gv = 0.5 * (t0 + tt.T(p, vr - 1, vc));
            ys[(2 * p) * kQyN + i] = (G.d_p * (G.minv * gu)) * xw + (G.d_p * (G.inv * gu)) * xc;
            ys[(2 * p + 1) * kQyN + i] = (G.d_p * (G.inv * gv)) * xn + (G.d_p * (G.minv * gv)) * xc;
        }
    }
    __syncthreads();
    // z = F y on the tile's cells and their east / south neighbours (held in registers, then over y)
    double zv[IZ][4];
    {
        const XTileT<kQyW, kQyH> yt{ys, r0 - 1, c0 - 1};
#pragma unroll
        for (int it = 0; it < IZ; ++it) {
            const int i = tid + it * 256;
            if (i >= kQzN) break;
            const int vr = r0 + i / kQzW, vc = c0 + i % kQzW;
            const typename FStencilFast::Co k = P.coeffs(P.nb(tt, vr, vc));
            P.rows4_co(vr, vc, k, P.weights(FStencilDev::Cell{{fu[it], fv[it]}}), yt, zv[it]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < IZ; ++it) {
        const int i = tid + it * 256;
        if (i >= kQzN) break;
#pragma unroll
        for (int f = 0; f < 4; ++f) ys[f * kQzN + i] = zv[it][f];
    }
    __syncthreads();
    // x_b = -(D z) on the tile (the pressure row: u at the west / east faces, v at the north / south faces, per phase)
    const XTileT<kQzW, kQzH> zt{ys, r0, c0};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int vr = r0 + tid / kQmW + 8 * m, vc = c0 + tid % kQmW;
        if (vr >= n || vc >= n) continue;
        const int32_t row = vr * n + vc;
        const typename Epi::P pe = epi.pre(row);
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const double t0 = tt.T(q, vr, vc);
            const double uC = (G.minv * (0.5 * (t0 + tt.T(q, vr, vc - 1)))) * zt.X(2 * q, vr, vc);
            const double uE = (G.inv * (0.5 * (t0 + tt.T(q, vr, vc + 1)))) * zt.X(2 * q, vr, vc + 1);
            const double vC = (G.inv * (0.5 * (t0 + tt.T(q, vr - 1, vc)))) * zt.X(2 * q + 1, vr, vc);
            const double vS = (G.minv * (0.5 * (t0 + tt.T(q, vr + 1, vc)))) * zt.X(2 * q + 1, vr + 1, vc);
            acc += uC;
            acc += uE;
            acc += vC;
            acc += vS;
        }
        epi(row, -acc, pe);
    }
}
// whole grid, one GPU: the staged window (tile + 2) wraps at most once
inline bool qmf_ok_n(int n) { return n >= kQxW && n >= kQxH; }
// The plan's Gt_F_G product by k_qmf: kernel option q13_mf, tolerance mode, one GPU, matrix-free F (fast rows) and D / G.
bool qmf_ok(const mpbp_schur_plan* p) {
    return KO().q13_mf && p->f_numerics == MPBP_NUMERICS_FAST && p->f_stencil && p->pg_stencil && !p->halo &&
           p->f_cell && p->f_uface && p->f_vface && qmf_ok_n(p->f_prm.n);
}
template <class Epi>
int launch_qmf(const mpbp_schur_plan* p, const double* xa, Epi epi, hipStream_t st) {
    FStencilDev Pd;
    int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &Pd);
    if (rc) return rc;
    PGDev G;
    rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &G);
    if (rc) return rc;
    const FStencilFast P{Pd};
    if (!qmf_ok_n(P.n) || !xa || xa == epi.y) return set_error(MPBP_ERR_ARG, "qmf: whole grid n >= 36, vectors");
    const int64_t tiles = (int64_t)((P.n + kQmW - 1) / kQmW) * ((P.n + kQmH - 1) / kQmH);
    k_qmf<Epi><<<(unsigned)tiles, 256, 0, st>>>(P, G, xa, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
}  // namespace

extern "C" {
int mpbp_svl_spmv(const mpbp_svl* V, const mpbp_csr* A, int32_t mode, const double* x, const double* z, double* y,
                  void* stream) {
    int rc = check_csr(A);
    if (!rc) rc = check_svl(V, A);
    if (rc) return rc;
    if (!x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "svl_spmv: bad vectors");
    return svl_spmv(V, A, mode, x, z, y, as_stream(stream));
}

int mpbp_svl_cheb_step(const mpbp_svl* V, const mpbp_csr* A, const double* x_in, const double* b, const double* diag,
                       double c1, double c2, double* d, const double* sub, double* x_out, void* stream) {
    int rc = check_csr(A);
    if (!rc) rc = check_svl(V, A);
    if (rc) return rc;
    if (!x_in || !b || !diag || !d || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "svl_cheb_step: bad vectors");
    return svl_cheb(V, A, x_in, b, diag, c1, c2, d, sub, x_out, as_stream(stream), 1, false);
}

int mpbp_q13_build(const mpbp_csr* Q, int32_t n, double* vals, void* stream) {
    int rc = check_csr(Q);
    if (rc) return rc;
    if (n < 5 || (int64_t)n * n > INT32_MAX / kQSlots || Q->nrows != n * n || Q->ncols != n * n || !vals)
        return set_error(MPBP_ERR_ARG, "q13_build: needs an n^2 x n^2 operator, n >= 5");
    const hipStream_t st = as_stream(stream);
    int* bad = nullptr;
    MPBP_HIP(hipMallocAsync((void**)&bad, sizeof(int), st));
    MPBP_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    k_q13_fill<<<grid_for((int64_t)n * n), kBlock, 0, st>>>(to_csr(Q), n * n, n, vals, bad);
    MPBP_HIP(hipGetLastError());
    int nbad = 0;
    MPBP_HIP(hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    MPBP_HIP(hipFreeAsync(bad, st));
    MPBP_HIP(hipStreamSynchronize(st));
    if (nbad) return set_error(MPBP_ERR_ARG, "q13_build: %d rows are not the 13-point diamond", nbad);
    return MPBP_OK;
}

int mpbp_q13_build_rows(const mpbp_csr* Q, int32_t n, int32_t row0, double* vals, void* stream) {
    int rc = check_csr(Q);
    if (rc) return rc;
    if (n < 5 || Q->nrows < n || Q->nrows % n || Q->nrows > (n + 2) * n || (int64_t)Q->nrows > INT32_MAX / kQSlots ||
        Q->ncols != n * n || !vals)
        return set_error(MPBP_ERR_ARG, "q13_build_rows: needs whole grid rows of an n^2-column operator, n >= 5");
    const hipStream_t st = as_stream(stream);
    int* bad = nullptr;
    MPBP_HIP(hipMallocAsync((void**)&bad, sizeof(int), st));
    MPBP_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    k_q13_fill<<<grid_for((int64_t)Q->nrows), kBlock, 0, st>>>(to_csr(Q), Q->nrows, n, vals, bad, row0);
    MPBP_HIP(hipGetLastError());
    int nbad = 0;
    MPBP_HIP(hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    MPBP_HIP(hipFreeAsync(bad, st));
    MPBP_HIP(hipStreamSynchronize(st));
    if (nbad) return set_error(MPBP_ERR_ARG, "q13_build_rows: %d rows are not the 13-point diamond", nbad);
    return MPBP_OK;
}

int mpbp_q13_asymmetry(int32_t n, const double* vals, double* out, void* stream) {
    if (n < 5 || (int64_t)n * n > INT32_MAX / kQSlots || !vals || !out) return set_error(MPBP_ERR_ARG, "q13_asymmetry: bad args");
    const hipStream_t st = as_stream(stream);
    unsigned long long* dev = nullptr;
    MPBP_HIP(hipMallocAsync((void**)&dev, 2 * sizeof(unsigned long long), st));
    MPBP_HIP(hipMemsetAsync(dev, 0, 2 * sizeof(unsigned long long), st));
    k_q13_asym<<<grid_for((int64_t)n * n), kBlock, 0, st>>>(n, vals, dev);
    MPBP_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    MPBP_HIP(hipMemcpyAsync(h, dev, sizeof(h), hipMemcpyDeviceToHost, st));
    MPBP_HIP(hipFreeAsync(dev, st));
    MPBP_HIP(hipStreamSynchronize(st));
    memcpy(out, h, sizeof(h));
    return MPBP_OK;
}

int mpbp_q13_spmv(int32_t n, const double* vals, int32_t mode, const double* x, const double* z, double* y,
                  void* stream) {
    if (n < 5 || (int64_t)n * n > INT32_MAX / kQSlots || !vals || !x || !y || (mode != MPBP_SPMV_STORE && !z))
        return set_error(MPBP_ERR_ARG, "q13_spmv: bad args");
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_q13(n, vals, x, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_q13(n, vals, x, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_q13(n, vals, x, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "q13_spmv: unknown mode %d", mode);
    }
}
}  // extern "C"
