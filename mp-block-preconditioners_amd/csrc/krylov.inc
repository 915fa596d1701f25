// Krylov orthogonalisation: the Gram-Schmidt kernels, reproducible (binned) dot products, DCGS2 and their C ABI.
// Needs only mpbp.hip's includes and its first section (set_error, MPBP_HIP, as_stream, kBlock, grid_for).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

// ================================================= Krylov orthogonalisation ====
// FGMRES's classical Gram-Schmidt passes over the Krylov basis V (k vectors of n doubles, row stride ld):
// h = V w (mpbp_gs_dot) and w_out = w - V^T h (mpbp_gs_update).  rocBLAS's gemv over a k x 5 M row-major basis
// streams at ~2 TB/s; these stream V once per pass at HBM speed.  Deterministic: the dot products are per-chunk
// partial sums (each workgroup's in a fixed tree order) added chunk after chunk by one thread per vector.
namespace {
constexpr int kGsVec = 8;      // basis vectors per dot-product workgroup
constexpr int kGsPer = 16;     // elements per thread per chunk
constexpr int kGsBatch = 4;    // elements whose loads are issued together
constexpr int kGsChunk = kBlock * kGsPer;
__global__ void __launch_bounds__(kBlock) k_gs_dot(const double* __restrict__ V, int64_t ld, int k,
                                                   const double* __restrict__ w, int64_t n, double* part) {
    const int64_t c = blockIdx.x;
    const int i0 = blockIdx.y * kGsVec;
    const int nv = min(kGsVec, k - i0);
    double acc[kGsVec];
#pragma unroll
    for (int v = 0; v < kGsVec; ++v) acc[v] = 0.0;
    for (int u = 0; u < kGsPer; u += kGsBatch) {
        double wv[kGsBatch], vv[kGsVec][kGsBatch];
#pragma unroll
        for (int q = 0; q < kGsBatch; ++q) {   // every load of the batch in flight at once
            const int64_t e = c * kGsChunk + (int64_t)(u + q) * kBlock + threadIdx.x;
            const bool ok = e < n;
            const int64_t ee = ok ? e : 0;
            wv[q] = ok ? w[ee] : 0.0;
#pragma unroll
            for (int v = 0; v < kGsVec; ++v) vv[v][q] = v < nv ? V[(int64_t)(i0 + v) * ld + ee] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kGsBatch; ++q)
#pragma unroll
            for (int v = 0; v < kGsVec; ++v) acc[v] += vv[v][q] * wv[q];
    }
    __shared__ double red[kGsVec][kBlock / 64];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < kGsVec; ++v) {
        double a = acc[v];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) red[v][wv_] = a;
    }
    __syncthreads();
    if (threadIdx.x < nv) {
        double a = 0.0;
        for (int q = 0; q < kBlock / 64; ++q) a += red[threadIdx.x][q];
        part[c * k + i0 + threadIdx.x] = a;
    }
}
// h[i] = the chunk partials of vector i, one workgroup per vector: strided per-thread sums, then a fixed tree.
__global__ void __launch_bounds__(kBlock) k_gs_sum(const double* part, int64_t nchunks, int k, double* h) {
    const int i = blockIdx.x;
    double a = 0.0;
    for (int64_t c = threadIdx.x; c < nchunks; c += kBlock) a += part[c * k + i];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    __shared__ double red[kBlock / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < kBlock / 64; ++q) t += red[q];
        h[i] = t;
    }
}
// (w and wo may alias: each thread reads w[e] before it writes wo[e], so neither is declared __restrict__)
__global__ void __launch_bounds__(kBlock) k_gs_update(const double* __restrict__ V, int64_t ld, int k,
                                                      const double* __restrict__ h, const double* w,
                                                      int64_t n, double* wo) {
    __shared__ double hs[256];
    for (int i = threadIdx.x; i < k; i += kBlock) hs[i] = h[i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    double a = 0.0;
    int i = 0;
    for (; i + 8 <= k; i += 8) {   // 8 basis rows' loads in flight, then added in order
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = V[(int64_t)(i + q) * ld + e];
#pragma unroll
        for (int q = 0; q < 8; ++q) a += v[q] * hs[i + q];
    }
    for (; i < k; ++i) a += V[(int64_t)i * ld + e] * hs[i];
    wo[e] = w[e] - a;
}
// ---- reproducible dot products: binned summation (Demmel & Nguyen's pre-rounding, 3 folds) ----
// Every term t = v w (|t| <= 2^E, E from the caller's bounds; N terms in the whole distributed vector) is split as
// t = q0 + q1 + q2 + (dropped): q_f = fl(sigma_f + r) - sigma_f with sigma_f = 1.5 * 2^(E + (f+1) L - 53 f), L >= log2 N + 1,
// r the remainder of the previous folds.  Each q_f is a multiple of ulp(sigma_f) and N of them sum to less than
// 2^53 such ulps, so every partial sum of a fold is EXACT: the fold sums -- and h = (S0 + S1) + S2 -- depend only on
// the set of terms, never on the order, the chunking, the launch configuration or the split of the vector over
// ranks (the sums of the ranks' fold sums are exact too).  FGMRES therefore computes the same bits on one GPU and
// on a row partition.  Accuracy: |h - sum t| <= N 2^(E + 3L - 159) + one rounding (about 2^-51 of the bound for
// N = 2^24), against the N eps sum|t| of a plain sum.  A fold whose sigma would be subnormal is skipped (q = 0).
constexpr int kRdVec = 4;      // basis vectors per workgroup
constexpr int kRdFolds = 3;
__device__ inline void rd_sigmas(double bound, int64_t ntot, double* sig) {
    int E = 0;
    (void)frexp(bound, &E);    // bound < 2^E
    const int L = 65 - __clzll((unsigned long long)(ntot > 0 ? ntot : 1));
    const bool finite = bound == bound && bound <= 1.7976931348623157e308;
#pragma unroll
    for (int f = 0; f < kRdFolds; ++f) {
        const int ex = E + (f + 1) * L - 53 * f;
        sig[f] = (!finite || (bound > 0.0 && E + L > 1023)) ? __longlong_as_double(0x7ff8000000000000LL)   // NaN / range
                 : !(bound > 0.0) ? 0.0                              // all terms 0: nothing to fold
                 : ex >= -1022 ? ldexp(1.5, ex) : 0.0;               // subnormal fold: skipped
    }
}
__device__ inline void rd_fold(double t, const double* sig, double* acc) {
    double r = t;
#pragma unroll
    for (int f = 0; f < kRdFolds; ++f) {
        const double q = (sig[f] + r) - sig[f];
        const double qq = sig[f] != 0.0 ? q : 0.0;
        acc[f] += qq;
        r -= qq;
    }
}
__global__ void __launch_bounds__(kBlock) k_rdot(const double* __restrict__ V, int64_t ld, int k,
                                                 const double* __restrict__ w, int64_t n, int64_t ntot,
                                                 const double* __restrict__ bound_v, const double* __restrict__ bound_w,
                                                 double* part) {
    const int64_t c = blockIdx.x;
    const int i0 = blockIdx.y * kRdVec;
    const int nv = min(kRdVec, k - i0);
    double sig[kRdVec][kRdFolds], acc[kRdVec][kRdFolds];
    const double bw = bound_w[0];
#pragma unroll
    for (int v = 0; v < kRdVec; ++v) {
        rd_sigmas(v < nv ? bound_v[i0 + v] * bw : 0.0, ntot, sig[v]);
#pragma unroll
        for (int f = 0; f < kRdFolds; ++f) acc[v][f] = 0.0;
    }
    for (int u = 0; u < kGsPer; u += kGsBatch) {
        double wv[kGsBatch], vv[kRdVec][kGsBatch];
#pragma unroll
        for (int q = 0; q < kGsBatch; ++q) {   // every load of the batch in flight at once
            const int64_t e = c * kGsChunk + (int64_t)(u + q) * kBlock + threadIdx.x;
            const bool ok = e < n;
            const int64_t ee = ok ? e : 0;
            wv[q] = ok ? w[ee] : 0.0;
#pragma unroll
            for (int v = 0; v < kRdVec; ++v) vv[v][q] = v < nv ? V[(int64_t)(i0 + v) * ld + ee] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kGsBatch; ++q)
#pragma unroll
            for (int v = 0; v < kRdVec; ++v) rd_fold(vv[v][q] * wv[q], sig[v], acc[v]);
    }
    // block reduction: exact additions, so the tree shape does not matter
    __shared__ double red[kRdVec * kRdFolds][kBlock / 64];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < kRdVec; ++v)
#pragma unroll
        for (int f = 0; f < kRdFolds; ++f) {
            double a = acc[v][f];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
            if (lane == 0) red[v * kRdFolds + f][wv_] = a;
        }
    __syncthreads();
    if (threadIdx.x < nv * kRdFolds) {
        double a = 0.0;
        for (int q = 0; q < kBlock / 64; ++q) a += red[threadIdx.x][q];
        part[c * (3 * (int64_t)k) + 3 * i0 + threadIdx.x] = a;
    }
}
// ---- DCGS2 (Gram-Schmidt with delayed re-orthogonalisation: Swirydowicz et al. 2020, Bielich et al. 2022) ----
// FGMRES iteration j holds q_0 .. q_{j-1} (orthonormal) and u_j (= V[j], projected once, not normalised); one pass over
// the basis forms the block product [V[0..j]] . [u_j, w] (w = A M u_j) -- the fold sums of both columns (k_rdot2) --
// and one more pass (k_dcgs2_update) re-orthogonalises and normalises u_j into q_j and projects w once into u_{j+1}:
// two passes over the basis per iteration instead of CGS2's four.  Scalars (k_dcgs2_coeffs, one thread, fixed order):
//   s = V[0..j-1] . u_j, alpha = u_j . u_j, z = V[0..j-1] . w, beta = u_j . w,
//   r = sqrt(alpha - s.s), q_j = (u_j - V s) / r, c = (beta - s.z) / r = q_j . w, u_{j+1} = w - V z - q_j c
// (j = 0: q_0 = u_0 is the normalised residual, r = 1).  Arnoldi: A Z[j] = w = V z + q_j c + u_{j+1}, and
// u_{j+1} = V' s' + r' q_{j+1} one iteration later, so column j of H is z + s', c + s'_j, r' (one iteration lagged).
// Bounds for the binned sums: |q_i| <= 1 (unit vectors), |u_{j+1}| <= (max|w| + sum |z_i| + |c|) (1 + 2^-40).
__global__ void __launch_bounds__(kBlock) k_rdot2(const double* __restrict__ V, int64_t ld, int k,
                                                  const double* __restrict__ u, const double* __restrict__ w, int64_t n,
                                                  int64_t ntot, const double* __restrict__ bound_v,
                                                  const double* __restrict__ bound_u, const double* __restrict__ bound_w,
                                                  double* part) {
    const int64_t c = blockIdx.x;
    const double bu = bound_u[0], bw = bound_w[0];
    __shared__ double red[kRdVec * 2 * kRdFolds][kBlock / 64];
    const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
    for (int i0 = 0; i0 < k; i0 += kRdVec) {   // the chunk's u and w re-read per group from L2; V streamed once
        const int nv = min(kRdVec, k - i0);
        double sig[kRdVec][2][kRdFolds], acc[kRdVec][2][kRdFolds];
#pragma unroll
        for (int v = 0; v < kRdVec; ++v) {
            const double b = v < nv ? bound_v[i0 + v] : 0.0;
            rd_sigmas(b * bu, ntot, sig[v][0]);
            rd_sigmas(b * bw, ntot, sig[v][1]);
#pragma unroll
            for (int f = 0; f < kRdFolds; ++f) acc[v][0][f] = acc[v][1][f] = 0.0;
        }
        for (int uu = 0; uu < kGsPer; uu += kGsBatch) {
            double uv[kGsBatch], wv[kGsBatch], vv[kRdVec][kGsBatch];
#pragma unroll
            for (int q = 0; q < kGsBatch; ++q) {
                const int64_t e = c * kGsChunk + (int64_t)(uu + q) * kBlock + threadIdx.x;
                const bool ok = e < n;
                const int64_t ee = ok ? e : 0;
                uv[q] = ok ? u[ee] : 0.0;
                wv[q] = ok ? w[ee] : 0.0;
#pragma unroll
                for (int v = 0; v < kRdVec; ++v) vv[v][q] = (v < nv && ok) ? V[(int64_t)(i0 + v) * ld + ee] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kGsBatch; ++q)
#pragma unroll
                for (int v = 0; v < kRdVec; ++v) {
                    rd_fold(vv[v][q] * uv[q], sig[v][0], acc[v][0]);
                    rd_fold(vv[v][q] * wv[q], sig[v][1], acc[v][1]);
                }
        }
#pragma unroll
        for (int v = 0; v < kRdVec; ++v)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int f = 0; f < kRdFolds; ++f) {
                    double a = acc[v][r][f];
                    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
                    if (lane == 0) red[(v * 2 + r) * kRdFolds + f][wv_] = a;
                }
        __syncthreads();
        if (threadIdx.x < nv * 2 * kRdFolds) {
            const int t = threadIdx.x, v = t / (2 * kRdFolds), r = (t / kRdFolds) & 1, f = t % kRdFolds;
            double a = 0.0;
            for (int q = 0; q < kBlock / 64; ++q) a += red[t][q];
            part[c * (6 * (int64_t)k) + r * 3 * (int64_t)k + 3 * (i0 + v) + f] = a;
        }
        __syncthreads();
    }
}
// hu[0..j], hw[0..j] from the fold sums (acc: 3 (j+1) for u, then 3 (j+1) for w); P = {r, 1 / r, c, bound of u_{j+1}}.
__global__ void k_dcgs2_coeffs(int j, const double* __restrict__ acc, const double* __restrict__ bound_w,
                               double* __restrict__ hu, double* __restrict__ hw, double* __restrict__ P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int k = j + 1;
    double ss = 0.0, sz = 0.0, b = bound_w[0];
    for (int i = 0; i < k; ++i) {
        hu[i] = (acc[3 * i] + acc[3 * i + 1]) + acc[3 * i + 2];
        hw[i] = (acc[3 * k + 3 * i] + acc[3 * k + 3 * i + 1]) + acc[3 * k + 3 * i + 2];
    }
    for (int i = 0; i < j; ++i) {
        ss = ss + hu[i] * hu[i];
        sz = sz + hu[i] * hw[i];
        b = b + fabs(hw[i]);
    }
    double r = 1.0, rinv = 1.0;
    if (j > 0) {
        const double d = hu[j] - ss;
        r = d > 0.0 ? sqrt(d) : 0.0;
        rinv = r > 0.0 ? 1.0 / r : 0.0;
    }
    const double cc = (hw[j] - sz) * rinv;
    b = ((b + fabs(cc)) * rinv) * (1.0 + 0x1p-40);   // u_{j+1} is stored scaled by 1 / r (k_dcgs2_update)
    P[0] = r;
    P[1] = rinv;
    P[2] = cc;
    P[3] = b;
}
// V[j] <- q_j = (V[j] - V[0..j-1]^T s) / r; V[j + 1] <- u_{j+1} = ((w - V[0..j-1]^T z) - q_j c) / r (both sums in basis
// order from 0.0, k_gs_update's operations; upd_w = 0: q_j only).  w = A M u_j was formed from the raw u_j (norm ~ r):
// scaling u_{j+1} by 1 / r keeps the raw vectors at the size of A M q_j instead of growing by ||A M|| per iteration
// (the Arnoldi column then belongs to Z[j] / r, fgmres's bookkeeping).
__global__ void __launch_bounds__(kBlock) k_dcgs2_update(double* __restrict__ V, int64_t ld, int j,
                                                         const double* __restrict__ hu, const double* __restrict__ hw,
                                                         const double* __restrict__ P, const double* __restrict__ w,
                                                         int64_t n, int upd_w) {
    __shared__ double ss[256], zs[256];
    for (int i = threadIdx.x; i < j; i += kBlock) {
        ss[i] = hu[i];
        zs[i] = hw[i];
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    double su = 0.0, sw = 0.0;
    int i = 0;
    for (; i + 8 <= j; i += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = V[(int64_t)(i + q) * ld + e];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            su += v[q] * ss[i + q];
            sw += v[q] * zs[i + q];
        }
    }
    for (; i < j; ++i) {
        const double v = V[(int64_t)i * ld + e];
        su += v * ss[i];
        sw += v * zs[i];
    }
    const double qv = (V[(int64_t)j * ld + e] - su) * P[1];
    V[(int64_t)j * ld + e] = qv;
    if (upd_w) V[(int64_t)(j + 1) * ld + e] = ((w[e] - sw) - qv * P[2]) * P[1];
}

// CGS2's first update and second projection in one kernel: wo = w - V^T h (k_gs_update's operations, same bits) and
// the exact fold sums of V[i] . wo (k_rdot's pre-rounding).  The extractors cannot wait for max|wo|, so they come from
// the a-priori bound B = (max|w| + sum_i bound_v[i] |h[i]|) (1 + 2^-40) >= max|wo| -- the same in every workgroup and
// on every rank (its inputs are global), so the fold sums stay exact and reproducible; the looser bound costs accuracy
// only below 2^-58 of it.  A workgroup updates its chunk (16 elements per thread, kept in LDS), then forms the
// products vector group by vector group as k_rdot does, re-reading the chunk's basis entries it has just streamed
// (from the L2 / MALL while they last) instead of a second full pass -- and wo is never re-read.
__global__ void __launch_bounds__(kBlock) k_gs_update_rdot(const double* __restrict__ V, int64_t ld, int k,
                                                           const double* __restrict__ h, const double* w, int64_t n,
                                                           int64_t ntot, const double* __restrict__ bound_v,
                                                           const double* __restrict__ bound_w, double* wo,
                                                           double* __restrict__ part) {
    __shared__ double hs[256];
    __shared__ double sg[256 * kRdFolds];
    __shared__ double red[kBlock / 64][kRdVec * kRdFolds];
    __shared__ double bnd;
    const int tid = threadIdx.x, lane = tid & 63, wq = tid >> 6;
    for (int i = tid; i < k; i += kBlock) hs[i] = h[i];
    __syncthreads();
    if (tid == 0) {
        double b = bound_w[0];
        for (int i = 0; i < k; ++i) b += bound_v[i] * fabs(hs[i]);
        bnd = b * (1.0 + 0x1p-40);
    }
    __syncthreads();
    for (int i = tid; i < k; i += kBlock) rd_sigmas(bound_v[i] * bnd, ntot, sg + kRdFolds * i);
    const int64_t c = blockIdx.x;
    __shared__ double w1[kGsChunk];   // the updated chunk, [u][thread]
    for (int u = 0; u < kGsPer; ++u) {   // the update, element by element (k_gs_update's order of operations)
        const int64_t e = c * kGsChunk + (int64_t)u * kBlock + tid;
        const bool ok = e < n;
        const int64_t ee = ok ? e : 0;
        double a = 0.0;
        int i = 0;
        for (; i + 8 <= k; i += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = V[(int64_t)(i + q) * ld + ee];
#pragma unroll
            for (int q = 0; q < 8; ++q) a += v[q] * hs[i + q];
        }
        for (; i < k; ++i) a += V[(int64_t)i * ld + ee] * hs[i];
        const double r = ok ? w[ee] - a : 0.0;
        w1[u * kBlock + tid] = r;
        if (ok) wo[ee] = r;
    }
    __syncthreads();   // (sg; each thread reads back only its own w1 entries)
    for (int i0 = 0; i0 < k; i0 += kRdVec) {   // the products, kRdVec basis vectors at a time (k_rdot's folds)
        const int nv = min(kRdVec, k - i0);
        double acc[kRdVec][kRdFolds], sig[kRdVec][kRdFolds];
#pragma unroll
        for (int v = 0; v < kRdVec; ++v)
#pragma unroll
            for (int f = 0; f < kRdFolds; ++f) {
                acc[v][f] = 0.0;
                sig[v][f] = v < nv ? sg[kRdFolds * (i0 + v) + f] : 0.0;
            }
        for (int u = 0; u < kGsPer; u += kGsBatch) {
            double vv[kRdVec][kGsBatch];
#pragma unroll
            for (int q = 0; q < kGsBatch; ++q) {
                const int64_t e = c * kGsChunk + (int64_t)(u + q) * kBlock + tid;
                const int64_t ee = e < n ? e : 0;
#pragma unroll
                for (int v = 0; v < kRdVec; ++v) vv[v][q] = v < nv ? V[(int64_t)(i0 + v) * ld + ee] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kGsBatch; ++q)
#pragma unroll
                for (int v = 0; v < kRdVec; ++v) rd_fold(vv[v][q] * w1[(u + q) * kBlock + tid], sig[v], acc[v]);
        }
#pragma unroll
        for (int v = 0; v < kRdVec; ++v)
#pragma unroll
            for (int f = 0; f < kRdFolds; ++f) {
                double x = acc[v][f];
                for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
                if (lane == 0) red[wq][kRdFolds * v + f] = x;
            }
        __syncthreads();
        if (tid < kRdFolds * nv) {   // the group's partials over the 4 waves (exact)
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < kBlock / 64; ++q) t += red[q][tid];
            part[c * (kRdFolds * (int64_t)k) + kRdFolds * i0 + tid] = t;
        }
        __syncthreads();
    }
}
// acc[j] = sum over chunks of part[c][j] (exact), one workgroup per fold sum
__global__ void __launch_bounds__(kBlock) k_rdot_sum(const double* part, int64_t nchunks, int k3, double* acc) {
    const int j = blockIdx.x;
    double a = 0.0;
    for (int64_t c = threadIdx.x; c < nchunks; c += kBlock) a += part[c * k3 + j];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    __shared__ double red[kBlock / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < kBlock / 64; ++q) t += red[q];
        acc[j] = t;
    }
}
__global__ void k_rdot_finish(int k, const double* acc, double* h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) h[i] = (acc[3 * i] + acc[3 * i + 1]) + acc[3 * i + 2];
}
// amax = max |x| (non-negative doubles order like their bit patterns; NaN's pattern exceeds every finite one)
// Eight loads in flight per thread, the maximum taken on the bit patterns, one atomic per workgroup (one per wave
// made every wave of a 5 M-entry vector queue on the same address: 65 us per call in the FGMRES loop).
__global__ void __launch_bounds__(kBlock) k_absmax(const double* __restrict__ x, int64_t n, unsigned long long* out) {
    __shared__ unsigned long long red[kBlock / 64];
    unsigned long long b = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; e + 7 * stride < n; e += 8 * stride) {
        double a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = x[e + u * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(a[u]));
            b = v > b ? v : b;
        }
    }
    for (; e < n; e += stride) {
        const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(x[e]));
        b = v > b ? v : b;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(b, off, 64);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) b = red[w] > b ? red[w] : b;
        atomicMax(out, b);
    }
}
}  // namespace

extern "C" {

int mpbp_gs_dot(const double* V, int64_t ld, int32_t k, const double* w, int64_t n, double* part, double* h,
                void* stream) {
    if (!V || !w || !h || !part || k < 1 || k > 256 || n < 1 || ld < n)
        return set_error(MPBP_ERR_ARG, "gs_dot: bad args (1 <= k <= 256, ld >= n)");
    const int64_t nchunks = (n + kGsChunk - 1) / kGsChunk;
    const dim3 grid((unsigned)nchunks, (unsigned)((k + kGsVec - 1) / kGsVec));
    k_gs_dot<<<grid, kBlock, 0, as_stream(stream)>>>(V, ld, k, w, n, part);
    MPBP_HIP(hipGetLastError());
    k_gs_sum<<<k, kBlock, 0, as_stream(stream)>>>(part, nchunks, k, h);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int64_t mpbp_gs_part_size(int64_t n, int32_t k) { return ((n + kGsChunk - 1) / kGsChunk) * (int64_t)k; }

int64_t mpbp_rdot_part_size(int64_t n, int32_t k) { return ((n + kGsChunk - 1) / kGsChunk) * 3 * (int64_t)k; }

int mpbp_rdot(const double* V, int64_t ld, int32_t k, const double* w, int64_t n, int64_t n_total,
              const double* bound_v, const double* bound_w, double* part, double* acc, void* stream) {
    if (!V || !w || !bound_v || !bound_w || !part || !acc || k < 1 || k > 256 || n < 0 || ld < n || n_total < n)
        return set_error(MPBP_ERR_ARG, "rdot: bad args (1 <= k <= 256, ld >= n, n_total >= n)");
    const hipStream_t st = as_stream(stream);
    if (n == 0) {
        MPBP_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 3 * (size_t)k, st));
        return MPBP_OK;
    }
    const int64_t nchunks = (n + kGsChunk - 1) / kGsChunk;
    const dim3 grid((unsigned)nchunks, (unsigned)((k + kRdVec - 1) / kRdVec));
    k_rdot<<<grid, kBlock, 0, st>>>(V, ld, k, w, n, n_total, bound_v, bound_w, part);
    MPBP_HIP(hipGetLastError());
    k_rdot_sum<<<3 * k, kBlock, 0, st>>>(part, nchunks, 3 * k, acc);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_rdot2(const double* V, int64_t ld, int32_t k, const double* u, const double* w, int64_t n, int64_t n_total,
               const double* bound_v, const double* bound_u, const double* bound_w, double* part, double* acc,
               void* stream) {
    if (!V || !u || !w || !bound_v || !bound_u || !bound_w || !part || !acc || k < 1 || k > 256 || n < 0 || ld < n ||
        n_total < n)
        return set_error(MPBP_ERR_ARG, "rdot2: bad args (1 <= k <= 256, ld >= n, n_total >= n)");
    const hipStream_t st = as_stream(stream);
    if (n == 0) {
        MPBP_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 6 * (size_t)k, st));
        return MPBP_OK;
    }
    const int64_t nchunks = (n + kGsChunk - 1) / kGsChunk;
    k_rdot2<<<(unsigned)nchunks, kBlock, 0, st>>>(V, ld, k, u, w, n, n_total, bound_v, bound_u, bound_w, part);
    MPBP_HIP(hipGetLastError());
    k_rdot_sum<<<6 * k, kBlock, 0, st>>>(part, nchunks, 6 * k, acc);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_dcgs2_update(double* V, int64_t ld, int32_t j, const double* acc, const double* bound_w, const double* w,
                      int64_t n, int32_t upd_w, double* hu, double* hw, double* P, void* stream) {
    if (!V || !acc || !bound_w || !hu || !hw || !P || (upd_w && !w) || j < 0 || j > 255 || n < 1 || ld < n)
        return set_error(MPBP_ERR_ARG, "dcgs2_update: bad args (0 <= j <= 255, ld >= n)");
    const hipStream_t st = as_stream(stream);
    k_dcgs2_coeffs<<<1, 64, 0, st>>>(j, acc, bound_w, hu, hw, P);
    MPBP_HIP(hipGetLastError());
    k_dcgs2_update<<<grid_for(n), kBlock, 0, st>>>(V, ld, j, hu, hw, P, w, n, upd_w);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_gs_update_rdot(const double* V, int64_t ld, int32_t k, const double* h, const double* w, int64_t n,
                        int64_t n_total, const double* bound_v, const double* bound_w, double* w_out, double* part,
                        double* acc, void* stream) {
    if (!V || !w || !h || !w_out || !bound_v || !bound_w || !part || !acc || k < 1 || k > 256 || n < 1 || ld < n ||
        n_total < n)
        return set_error(MPBP_ERR_ARG, "gs_update_rdot: bad args (1 <= k <= 256, ld >= n >= 1, n_total >= n)");
    const hipStream_t st = as_stream(stream);
    const int64_t nchunks = (n + kGsChunk - 1) / kGsChunk;
    k_gs_update_rdot<<<(unsigned)nchunks, kBlock, 0, st>>>(V, ld, k, h, w, n, n_total, bound_v, bound_w, w_out, part);
    MPBP_HIP(hipGetLastError());
    k_rdot_sum<<<3 * k, kBlock, 0, st>>>(part, nchunks, 3 * k, acc);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_rdot_finish(int32_t k, const double* acc, double* h, void* stream) {
    if (!acc || !h || k < 1) return set_error(MPBP_ERR_ARG, "rdot_finish: bad args");
    k_rdot_finish<<<grid_for(k), kBlock, 0, as_stream(stream)>>>(k, acc, h);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_absmax(const double* x, int64_t n, double* amax, void* stream) {
    if (!amax || n < 0 || (n > 0 && !x)) return set_error(MPBP_ERR_ARG, "absmax: bad args");
    const hipStream_t st = as_stream(stream);
    MPBP_HIP(hipMemsetAsync(amax, 0, sizeof(double), st));
    if (n == 0) return MPBP_OK;
    const int64_t blocks = (n + kBlock * 16 - 1) / (kBlock * 16);
    k_absmax<<<(unsigned)(blocks < 1024 ? blocks : 1024), kBlock, 0, st>>>(x, n, reinterpret_cast<unsigned long long*>(amax));
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_gs_update(const double* V, int64_t ld, int32_t k, const double* h, const double* w, int64_t n, double* w_out,
                   void* stream) {
    if (!V || !w || !h || !w_out || k < 1 || k > 256 || n < 1 || ld < n)
        return set_error(MPBP_ERR_ARG, "gs_update: bad args (1 <= k <= 256, ld >= n)");
    k_gs_update<<<grid_for(n), kBlock, 0, as_stream(stream)>>>(V, ld, k, h, w, n, w_out);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

}  // extern "C"
