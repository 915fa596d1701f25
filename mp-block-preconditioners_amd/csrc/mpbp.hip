// libmpbp -- MI355X (gfx950) HIP kernels + C ABI for the multiphase-Stokes
// block-preconditioner apply.  Header: include/mpbp.h.  Design: DESIGN.md.
//
// Built with -ffp-contract=off: every kernel performs the IEEE operations of the
// sequential checker oracle/csr_oracle.c in the same order (row sums left to
// right from 0.0, no fused multiply-add), so results are bit-identical to it.
//
// This file is the one translation unit.  It holds the prelude and the device kernels up to the marching kernels; the
// tiled F, pressure-side and fused multigrid kernels, the launchers, the C ABI and the host-side algorithms live
// in the csrc/*.inc fragments included at its end, in this order (map: DESIGN.md section 4).
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "mpbp.h"

namespace {

thread_local char g_err[1024] = "";
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// Kernel choices (mpbp_kernel_opts, include/mpbp.h): the process defaults (mpbp_set_*), and the choices of the plan
// being applied -- mpbp_schur_apply / mpbp_mg_solve install their plan's copy for the duration of the call (OptsScope),
// so two preconditioners with different choices coexist and a captured graph holds its own plan's choices.
// kOpts is the one table of them: line i is the struct's word i (the static_assert below), with the default and the
// lowest and highest value a setter or a plan may hold.  g_defaults, check_opts and the mpbp_set_* entry points
// (set_default) read it.  gtg_tpb alone is no interval: 256 or 512, its two ends (check_opts says so).
// Measured defaults: march_rows 0 = the count that fills one round of workgroups (256^2 1 row -> 13.5k applies/s vs
// 7.6k at 4; 1024^2 4; 2048^2 16 -> 753 vs 727).
struct KOpt {
    size_t offset;
    const char* name;
    int32_t def, lo, hi;
};
#define MPBP_KOPT(f, def, lo, hi) {offsetof(mpbp_kernel_opts, f), #f, def, lo, hi}
constexpr KOpt kOpts[] = {
    MPBP_KOPT(march_rows, 0, 0, 4096),
    MPBP_KOPT(init_diag, 1, 0, 1),
    MPBP_KOPT(f_pair, 1, 0, 1),
    MPBP_KOPT(f_direct, 0, 0, 1),
    MPBP_KOPT(gtg_fused, 1, 0, 1),
    MPBP_KOPT(gtg_tpb, 512, 256, 512),
    MPBP_KOPT(gtg_drhs, 1, 0, 1),
    MPBP_KOPT(q13_sym, 1, 0, 1),
    MPBP_KOPT(f_tile, 1, 0, 1),
    MPBP_KOPT(f_solve, 1, 0, 1),
    MPBP_KOPT(mg_galerkin_mf, 2, 0, 2),
    MPBP_KOPT(mg_galerkin_mf_p, 1, 0, 1),
    MPBP_KOPT(pg_direct, 1, 0, 1),
    MPBP_KOPT(mg_group_rows, 65536, 0, INT32_MAX),
    MPBP_KOPT(mg_svl, 1, 0, 1),
    MPBP_KOPT(mg_mf_transfer, 1, 0, 1),
    MPBP_KOPT(csr_table, 1, 0, 1),
    MPBP_KOPT(mg_fuse_l0, 1, 0, 1),
    MPBP_KOPT(mg_coarse_tree, 0, 0, 1),
    MPBP_KOPT(f_solve_tile, 1, 0, 1),
    MPBP_KOPT(q13_mf, 0, 0, 1),
    MPBP_KOPT(mg_fuse_small, 1, 0, 1),
    MPBP_KOPT(gtg_solve_tile, 1, 0, 1),
};
#undef MPBP_KOPT
constexpr size_t kNumOpts = sizeof(kOpts) / sizeof(kOpts[0]);
constexpr bool opts_cover_struct() {   // nothing skipped, doubled or out of order
    for (size_t i = 0; i < kNumOpts; ++i)
        if (kOpts[i].offset != i * sizeof(int32_t)) return false;
    return true;
}
static_assert(kNumOpts == (sizeof(mpbp_kernel_opts) - sizeof(mpbp_kernel_opts::reserved)) / sizeof(int32_t) &&
                  opts_cover_struct(),
              "kOpts needs one line per field of mpbp_kernel_opts, in struct order");
// the struct as its int32 words (it holds nothing else: the static_assert above)
inline int32_t* opt_words(mpbp_kernel_opts& o) { return reinterpret_cast<int32_t*>(&o); }
inline const int32_t* opt_words(const mpbp_kernel_opts& o) { return reinterpret_cast<const int32_t*>(&o); }
inline mpbp_kernel_opts default_opts() {
    mpbp_kernel_opts o{};
    for (size_t i = 0; i < kNumOpts; ++i) opt_words(o)[i] = kOpts[i].def;
    return o;
}
mpbp_kernel_opts g_defaults = default_opts();
thread_local const mpbp_kernel_opts* t_opts = nullptr;
inline const mpbp_kernel_opts& KO() { return t_opts ? *t_opts : g_defaults; }
struct OptsScope {   // installs a plan's kernel choices (when it has its own) for one entry-point call
    const mpbp_kernel_opts* prev;
    explicit OptsScope(const mpbp_kernel_opts* o) : prev(t_opts) {
        if (o) t_opts = o;
    }
    ~OptsScope() { t_opts = prev; }
};
inline int pg_rows() { return KO().march_rows; }   // rows per workgroup of the D / G / Gt_G marching kernels: as F
// a plan's kernel choices must be values the setters accept
inline int check_opts(const mpbp_kernel_opts* o, const char* who) {
    if (!o) return MPBP_OK;
    bool ok = o->gtg_tpb == 256 || o->gtg_tpb == 512;
    for (size_t i = 0; i < kNumOpts; ++i)
        ok = ok && opt_words(*o)[i] >= kOpts[i].lo && opt_words(*o)[i] <= kOpts[i].hi;
    return ok ? MPBP_OK : set_error(MPBP_ERR_ARG, "%s: kernel options out of range", who);
}
// the body of every mpbp_set_*: the process default of the field at `offset`, refused outside its line's range
inline int set_default(size_t offset, int32_t v) {
    const KOpt& k = kOpts[offset / sizeof(int32_t)];
    if (v < k.lo || v > k.hi) return set_error(MPBP_ERR_ARG, "%s must be in [%d, %d]", k.name, k.lo, k.hi);
    opt_words(g_defaults)[offset / sizeof(int32_t)] = v;
    return MPBP_OK;
}

#define MPBP_HIP(call)                                                                      \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return set_error(MPBP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));         \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kBlock = 256;                    // 4 wave64 per workgroup, one row per thread

inline int grid_for(int64_t n, int block = kBlock) { return (int)((n + block - 1) / block); }

// Cache policy of the once-touched streams.  The SELL and CSR kernels read their matrix (touched once per SpMV)
// and write their result with nontemporal hints (+2-4 % on the 1024^2 A SpMV); the stencil kernels keep
// default-policy loads and stores (their x / b / d vectors are re-read by the next sweep from the cache;
// nontemporal costs them 3-7 %).
constexpr bool kSellNT = true, kCsrNT = true;
template <class T>
__device__ inline T ld_stream(const T* p) { return *p; }
template <bool NT = false, class T>
__device__ inline void st_stream(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ inline double2 ld_matrix(const double2* p) {
    if constexpr (NT) {
        const f64x2 v = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(p));
        return make_double2(v.x, v.y);
    } else {
        return *p;
    }
}
template <bool NT>
__device__ inline int2 ld_matrix(const int2* p) {
    if constexpr (NT) {
        const i32x2 v = __builtin_nontemporal_load(reinterpret_cast<const i32x2*>(p));
        return make_int2(v.x, v.y);
    } else {
        return *p;
    }
}

// ================================================================== theta ====
// thn(y, x) = 0.25 sin(2 pi x) sin(2 pi y) + 0.5 -- preconditioner.py:9-11
__device__ inline double thn_fn(double y, double x) {
    const double two_pi = 2.0 * 3.141592653589793;
    return 0.25 * sin(two_pi * x) * sin(two_pi * y) + 0.5;
}

__global__ void k_theta(int n, double* cell, double* uface, double* vface) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * n) return;
    const int r = (int)(i / n), c = (int)(i % n);
    const double dx = 1.0 / n, dy = 1.0 / n;
    cell[i] = thn_fn(-(r + 0.5) * dy, (c + 0.5) * dx);   // get_thn_vals cell centres
    uface[i] = thn_fn(-(r + 0.5) * dy, c * dx);          // w_thn, u rows (preconditioner.py:325)
    vface[i] = thn_fn((double)(-r) * dy, (c + 0.5) * dx);  // w_thn, v rows (preconditioner.py:326)
}

// =============================================================== stencils ====
// The reference assigns into dense matrices; a later write to the same (row, col)
// replaces the earlier one (n <= 2 only).  RowBuf restates that: last write wins.
struct RowBuf {
    int m;
    int32_t col[16];
    double val[16];
};

__device__ inline void put(RowBuf& w, int32_t col, double v) {
    for (int k = 0; k < w.m; ++k)
        if (w.col[k] == col) { w.val[k] = v; return; }
    w.col[w.m] = col;
    w.val[w.m] = v;
    ++w.m;
}

__device__ inline void sort_row(RowBuf& w) {
    for (int i = 1; i < w.m; ++i) {
        const int32_t cj = w.col[i];
        const double cv = w.val[i];
        int t = i - 1;
        while (t >= 0 && w.col[t] > cj) { w.col[t + 1] = w.col[t]; w.val[t + 1] = w.val[t]; --t; }
        w.col[t + 1] = cj;
        w.val[t + 1] = cv;
    }
}

// Periodic cell-centred volume fraction of one phase (ths = 1 - thn, preconditioner.py:74-81).
struct Phase {
    int n;
    const double* cell;
    int s;
    // Periodic index for a in [-1, n]: every stencil offset is +-1 (no integer division).
    __device__ int wrap(int a) const { return a < 0 ? a + n : (a >= n ? a - n : a); }
    __device__ int32_t idx(int r, int c) const { return wrap(r) * n + wrap(c); }
    __device__ double T(int r, int c) const { const double v = cell[idx(r, c)]; return s ? 1.0 - v : v; }
};

// L rows of one phase (2N x 2N) and the XI diagonal entry of that row.
// u rows: preconditioner.py:100-179 ; v rows: preconditioner.py:240-295 ; XI: :124-125.
__device__ void phase_L_row(const Phase& g, double xi, int32_t i, RowBuf& w, double& xi_ii) {
    const int n = g.n;
    const int32_t N = n * n;
    const double dx = 1.0 / n, dy = 1.0 / n;
    w.m = 0;
    if (i < N) {
        const int r = i / n, c = i % n;
        const double tij = g.T(r, c - 1), tip1j = g.T(r, c);
        const double tijp1 = g.T(r - 1, c - 1), tip1jp1 = g.T(r - 1, c);
        const double tijm1 = g.T(r + 1, c - 1), tip1jm1 = g.T(r + 1, c);
        const double iph_jph = 0.25 * (tij + tijp1 + tip1jp1 + tip1j);
        const double iph_jmh = 0.25 * (tij + tip1j + tijm1 + tip1jm1);
        const double iph_j = 0.5 * (tij + tip1j);
        xi_ii = xi * iph_j * (1.0 - iph_j);
        put(w, i, 1.0 / (dx * dx) * (-tip1j - tij) + 1.0 / (dy * dy) * (-iph_jph - iph_jmh));
        put(w, N + g.idx(r, c), 1.0 / (dx * dy) * (-tip1j + iph_jph));
        put(w, g.idx(r, c - 1), 1.0 / (dx * dx) * (tij));
        put(w, g.idx(r, c + 1), tip1j / (dx * dx));
        put(w, g.idx(r - 1, c), 1.0 / (dy * dy) * (iph_jph));
        put(w, g.idx(r + 1, c), 1.0 / (dy * dy) * (iph_jmh));
        put(w, N + g.idx(r, c - 1), 1.0 / (dy * dx) * (tij - iph_jph));
        put(w, N + g.idx(r + 1, c - 1), 1.0 / (dy * dx) * (iph_jmh - tij));
        put(w, N + g.idx(r + 1, c), 1.0 / (dx * dy) * (tip1j - iph_jmh));
    } else {
        const int32_t k = i - N;
        const int r = k / n, c = k % n;
        const double ip1_jph = 0.5 * (g.T(r, c) + g.T(r - 1, c));   // set in the u loop (:125)
        xi_ii = xi * ip1_jph * (1.0 - ip1_jph);
        const double tij = g.T(r, c), tip1j = g.T(r, c + 1);
        const double tijp1 = g.T(r - 1, c), tip1jp1 = g.T(r - 1, c + 1);
        const double tim1j = g.T(r, c - 1), tim1jp1 = g.T(r - 1, c - 1);
        const double imh_jph = 0.25 * (tim1j + tim1jp1 + tij + tijp1);
        const double iph_jph = 0.25 * (tij + tip1j + tijp1 + tip1jp1);
        put(w, i, -1.0 / (dy * dy) * (tijp1 + tij) - 1.0 / (dx * dx) * (iph_jph + imh_jph));
        put(w, N + g.idx(r, c - 1), 1.0 / (dx * dx) * imh_jph);
        put(w, N + g.idx(r, c + 1), 1.0 / (dx * dx) * iph_jph);
        put(w, N + g.idx(r - 1, c), 1.0 / (dy * dy) * tijp1);
        put(w, N + g.idx(r + 1, c), 1.0 / (dy * dy) * tij);
        put(w, k, 1.0 / (dx * dy) * (imh_jph - tij));
        put(w, g.idx(r, c + 1), 1.0 / (dy * dx) * (tij - iph_jph));
        put(w, g.idx(r - 1, c), 1.0 / (dy * dx) * (tijp1 - imh_jph));
        put(w, g.idx(r - 1, c + 1), 1.0 / (dy * dx) * (iph_jph - tijp1));
    }
    sort_row(w);
}

// G rows of one phase (2N x N), preconditioner.py:203-219.
__device__ void phase_G_row(const Phase& g, int32_t i, RowBuf& w) {
    const int n = g.n;
    const int32_t N = n * n;
    const double dx = 1.0 / n, dy = 1.0 / n;
    w.m = 0;
    if (i < N) {
        const int r = i / n, c = i % n;
        const double imh_j = 0.5 * (g.T(r, c) + g.T(r, c - 1));
        put(w, i, (1.0 / dx) * imh_j);
        put(w, g.idx(r, c - 1), -(1.0 / dx) * imh_j);
    } else {
        const int32_t k = i - N;
        const int r = k / n, c = k % n;
        const double i_jph = 0.5 * (g.T(r, c) + g.T(r - 1, c));
        put(w, k, -(1.0 / dy) * i_jph);
        put(w, g.idx(r - 1, c), (1.0 / dy) * i_jph);
    }
    sort_row(w);
}

// D rows of one phase (N x 2N), preconditioner.py:221-238.
__device__ void phase_D_row(const Phase& g, int32_t k, RowBuf& w) {
    const int n = g.n;
    const int32_t N = n * n;
    const double dx = 1.0 / n, dy = 1.0 / n;
    const int r = k / n, c = k % n;
    const double tij = g.T(r, c);
    const double iph_j = 0.5 * (tij + g.T(r, c + 1));
    const double imh_j = 0.5 * (tij + g.T(r, c - 1));
    const double i_jph = 0.5 * (tij + g.T(r - 1, c));
    const double i_jmh = 0.5 * (tij + g.T(r + 1, c));
    w.m = 0;
    put(w, g.idx(r, c + 1), 1.0 / dx * iph_j);
    put(w, k, -1.0 / dx * imh_j);
    put(w, N + k, 1.0 / dy * i_jph);
    put(w, N + g.idx(r + 1, c), -1.0 / dy * i_jmh);
    sort_row(w);
}

struct StokesDev {
    int n;
    double xi, eta_n, eta_s, c, d_u, d_p, d_div;
    const double* cell;
    const double* uface;
    const double* vface;
};

__device__ inline void append(RowBuf& o, int32_t col, double v) {
    o.col[o.m] = col;
    o.val[o.m] = v;
    ++o.m;
}

// F row R of [u_n, v_n, u_s, v_s]: F = XI + d_u blockdiag(eta_n L_n, eta_s L_s)
// (preconditioner.py:310, 315-337).  Columns come out sorted.
__device__ void F_row(const StokesDev& P, int32_t R, RowBuf& o) {
    const int32_t N = P.n * P.n;
    const int p = R >= 2 * N;
    const int32_t i = R - p * 2 * N;
    const Phase g{P.n, P.cell, p};
    RowBuf L;
    double xi_ii;
    phase_L_row(g, P.xi, i, L, xi_ii);
    // Face tables are absent when only the pattern is counted.
    const double th = !P.uface ? 0.0 : (i < N) ? P.uface[i] : P.vface[i - N];
    const double w = p ? P.c * (1.0 - th) : P.c * th;          // w_ths = c*ths, w_thn = c*thn
    const double eta = p ? P.eta_s : P.eta_n;
    const int32_t off = p * 2 * N, other = (1 - p) * 2 * N;
    o.m = 0;
    if (p == 1) append(o, other + i, P.d_u * xi_ii);              // d_u * XI_s (cross block)
    for (int k = 0; k < L.m; ++k) {
        double v = P.d_u * (eta * L.val[k]);
        if (L.col[k] == i) v = (w - P.d_u * xi_ii) + v;           // (w - d_u XI) + d_u eta L
        append(o, off + L.col[k], v);
    }
    if (p == 0) append(o, other + i, P.d_u * xi_ii);              // d_u * XI_n (cross block)
}

__device__ void build_row(const StokesDev& P, int op, int32_t R, RowBuf& o) {
    const int32_t N = P.n * P.n;
    RowBuf t;
    double xi_ii;
    o.m = 0;
    switch (op) {
    case MPBP_OP_A:
        if (R < 4 * N) {
            F_row(P, R, o);
            const int p = R >= 2 * N;
            phase_G_row(Phase{P.n, P.cell, p}, R - p * 2 * N, t);
            for (int k = 0; k < t.m; ++k) append(o, 4 * N + t.col[k], P.d_p * t.val[k]);
        } else {
            const int32_t q = R - 4 * N;
            phase_D_row(Phase{P.n, P.cell, 0}, q, t);
            for (int k = 0; k < t.m; ++k) append(o, t.col[k], P.d_div * t.val[k]);
            phase_D_row(Phase{P.n, P.cell, 1}, q, t);
            for (int k = 0; k < t.m; ++k) append(o, 2 * N + t.col[k], P.d_div * t.val[k]);
        }
        break;
    case MPBP_OP_F:
        F_row(P, R, o);
        break;
    case MPBP_OP_D:
        phase_D_row(Phase{P.n, P.cell, 0}, R, t);
        for (int k = 0; k < t.m; ++k) append(o, t.col[k], t.val[k]);
        phase_D_row(Phase{P.n, P.cell, 1}, R, t);
        for (int k = 0; k < t.m; ++k) append(o, 2 * N + t.col[k], t.val[k]);
        break;
    case MPBP_OP_G: {
        const int p = R >= 2 * N;
        phase_G_row(Phase{P.n, P.cell, p}, R - p * 2 * N, t);
        for (int k = 0; k < t.m; ++k) append(o, t.col[k], P.d_p * t.val[k]);
        break;
    }
    case MPBP_OP_L_N:
    case MPBP_OP_L_S:
        phase_L_row(Phase{P.n, P.cell, op == MPBP_OP_L_S}, P.xi, R, o, xi_ii);
        break;
    case MPBP_OP_D_N:
    case MPBP_OP_D_S:
        phase_D_row(Phase{P.n, P.cell, op == MPBP_OP_D_S}, R, o);
        break;
    case MPBP_OP_G_N:
    case MPBP_OP_G_S:
        phase_G_row(Phase{P.n, P.cell, op == MPBP_OP_G_S}, R, o);
        break;
    case MPBP_OP_XI_N:
    case MPBP_OP_XI_S:
        phase_L_row(Phase{P.n, P.cell, op == MPBP_OP_XI_S}, P.xi, R, t, xi_ii);
        append(o, R, xi_ii);
        break;
    default:
        break;
    }
}

// rows (optional): the operator rows to assemble, in order (a rank's owned + ghost rows); the output CSR's row i is
// operator row rows[i] with its global columns.  NULL: every row.
__global__ void k_stokes_count(StokesDev P, int op, int64_t nrows, int32_t* row_nnz, const int32_t* rows = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    RowBuf o;
    build_row(P, op, rows ? rows[i] : (int32_t)i, o);
    row_nnz[i] = o.m;
}

__global__ void k_stokes_fill(StokesDev P, int op, int64_t nrows, const int32_t* rp, int32_t* ci,
                              double* va, const int32_t* rows = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    RowBuf o;
    build_row(P, op, rows ? rows[i] : (int32_t)i, o);
    const int32_t base = rp[i];
    for (int k = 0; k < o.m; ++k) {
        ci[base + k] = o.col[k];
        va[base + k] = o.val[k];
    }
}

// One 1024-thread workgroup scans the whole array in 1024-element chunks (setup only).
// Exclusive scan of row counts into row_ptr (int64 running sums, so an int32 overflow is detected).
// Three passes over tiles of kScanTile counts: tile sums; one workgroup scans the tile sums (and writes
// row_ptr[n] = total); every tile then scans its counts from LDS and adds its offset.
constexpr int kScanTile = 4096;   // 256 threads x 16 counts

// Inclusive scan of one value per thread over a 256-thread workgroup; *sum = the workgroup's total.
__device__ inline long long block_scan256(long long x, long long* wsum, long long* sum) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    long long off = 0;
    for (int w = 0; w < wid; ++w) off += wsum[w];
    *sum = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return x + off;
}

// Tile t's counts into LDS (coalesced; zeros past n).
__device__ inline void scan_load_tile(const int32_t* in, int64_t n, int32_t* tile) {
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    for (int i = threadIdx.x; i < kScanTile; i += 256) tile[i] = base + i < n ? in[base + i] : 0;
    __syncthreads();
}

__global__ void __launch_bounds__(256) k_scan_tiles(const int32_t* in, int64_t n, long long* tile_sum) {
    __shared__ int32_t tile[kScanTile];
    __shared__ long long wsum[4];
    scan_load_tile(in, n, tile);
    long long s = 0;
    for (int i = 0; i < 16; ++i) s += tile[threadIdx.x * 16 + i];
    long long tot;
    block_scan256(s, wsum, &tot);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// In place: tile_sum[t] -> exclusive prefix of the tile sums; out[n] = total = *total.
__global__ void __launch_bounds__(256) k_scan_offsets(long long* tile_sum, int64_t ntiles, int32_t* out, int64_t n,
                                                      long long* total) {
    __shared__ long long wsum[4];
    long long carry = 0;
    for (int64_t base = 0; base < ntiles; base += 256) {
        const int64_t i = base + threadIdx.x;
        const long long v = i < ntiles ? tile_sum[i] : 0;
        long long sum;
        const long long inc = block_scan256(v, wsum, &sum);
        if (i < ntiles) tile_sum[i] = carry + inc - v;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        out[n] = (int32_t)carry;
        *total = carry;
    }
}

__global__ void __launch_bounds__(256) k_scan_apply(const int32_t* in, int64_t n, const long long* tile_off,
                                                    int32_t* out) {
    __shared__ int32_t tile[kScanTile];
    __shared__ long long wsum[4];
    scan_load_tile(in, n, tile);
    int32_t c[16];
    long long s = 0;
    for (int i = 0; i < 16; ++i) {
        c[i] = tile[threadIdx.x * 16 + i];
        s += c[i];
    }
    long long tot;
    long long run = tile_off[blockIdx.x] + block_scan256(s, wsum, &tot) - s;
    for (int i = 0; i < 16; ++i) {   // exclusive values back into the tile (this thread's own slots)
        tile[threadIdx.x * 16 + i] = (int32_t)run;
        run += c[i];
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    for (int i = threadIdx.x; i < kScanTile; i += 256)
        if (base + i < n) out[base + i] = tile[i];
}

// ================================================================ SpGEMM ====
struct Csr {
    const int32_t* rp;
    const int32_t* ci;
    const double* va;
    int32_t ncols = 0;   // set by to_csr (the uniform CSR path's x buffer descriptor); 0 = unknown
};

constexpr int kSpgemmMaxW = 64;
constexpr int kSpgemmWideW = 128;   // the wide forms' output rows (mpbp_*_wide): Galerkin rows below an odd level reach 86

// Row r of A*B: first-touch order over (A row order, B row order), then sorted by column.
// Same operation order as oracle/csr_oracle.c:row_product.
template <int W = kSpgemmMaxW>
__device__ int spgemm_row(const Csr A, const Csr B, int32_t r, int32_t* cols, double* vals) {
    int m = 0;
    for (int32_t ka = A.rp[r]; ka < A.rp[r + 1]; ++ka) {
        const double a = A.va[ka];
        const int32_t k = A.ci[ka];
        for (int32_t kb = B.rp[k]; kb < B.rp[k + 1]; ++kb) {
            const int32_t j = B.ci[kb];
            const double v = a * B.va[kb];
            int t = 0;
            while (t < m && cols[t] != j) ++t;
            if (t < m) {
                vals[t] += v;
            } else {
                if (m == W) return -1;
                cols[m] = j;
                vals[m] = v;
                ++m;
            }
        }
    }
    for (int i = 1; i < m; ++i) {
        const int32_t cj = cols[i];
        const double cv = vals[i];
        int t = i - 1;
        while (t >= 0 && cols[t] > cj) { cols[t + 1] = cols[t]; vals[t + 1] = vals[t]; --t; }
        cols[t + 1] = cj;
        vals[t + 1] = cv;
    }
    return m;
}

template <int W = kSpgemmMaxW>
__global__ void k_spgemm_count(Csr A, Csr B, int32_t nrows, int32_t* row_nnz, int* overflow) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    int32_t cols[W];
    double vals[W];
    const int m = spgemm_row<W>(A, B, r, cols, vals);
    if (m < 0) { atomicAdd(overflow, 1); row_nnz[r] = 0; }
    else row_nnz[r] = m;
}

template <int W = kSpgemmMaxW>
__global__ void k_spgemm_fill(Csr A, Csr B, int32_t nrows, double alpha, const int32_t* crp,
                              int32_t* cci, double* cva) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    int32_t cols[W];
    double vals[W];
    const int m = spgemm_row<W>(A, B, r, cols, vals);
    const int32_t base = crp[r];
    for (int k = 0; k < m; ++k) {
        cci[base + k] = cols[k];
        cva[base + k] = alpha * vals[k];
    }
}

// ------------------------------------------------ values-only products into a known pattern ----
// One wavefront per output row, lane t owning the row's entry t (its column read from C.col_idx): every product of the
// row is broadcast to the wave and the one lane whose column matches adds it, so each entry sees its products in
// spgemm_row's (A row order, B row order) traversal and holds spgemm_row's bits.  A triple product's inner row is
// built the same way into the lanes (first-touch order), scaled once and handed on through cross-lane reads -- it never
// reaches memory.  No atomics on values, no private arrays, no scratch, no LDS allocation.
struct RCsr {
    const int32_t* rp;
    const int32_t* ci;
    const double* va;
    int32_t nrows, ncols;
    int64_t nnz;
};

constexpr int kRefillLong = 1;      // an output or inner row holds more than kSpgemmMaxW entries
constexpr int kRefillMissing = 2;   // a product's column is not in C's row
constexpr int kRefillIndex = 4;     // a row extent or column index outside its array
constexpr int kRefillWide = 8;      // the wide form: an output row holds more than kSpgemmWideW entries

// lane `src` (wave-uniform) of v
__device__ inline int32_t lane_get(int32_t v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ inline double lane_get(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src),
                            __builtin_amdgcn_readlane(__double2loint(v), src));
}

// [a, b) of row r (wave-uniform), false when it does not lie inside the entry arrays
__device__ inline bool row_extent(const RCsr& M, int32_t r, int32_t& a, int32_t& b) {
    a = M.rp[r];
    b = M.rp[r + 1];
    return a >= 0 && a <= b && (int64_t)b <= M.nnz;
}

// The wave's row: lane t < m holds entry t (col, val; hit: it has received a product).  m is wave-uniform.
struct WaveRow {
    int32_t col;
    double val;
    bool hit;
    int m;
};

// One product (j, v), both wave-uniform.  APPEND: an unseen column becomes entry m (first-touch order, spgemm_row);
// otherwise the pattern is fixed and an unseen column is an error.
template <bool APPEND>
__device__ inline void wave_feed(WaveRow& w, int lane, int32_t j, double v, int& err) {
    const bool mine = lane < w.m && w.col == j;
    if (__builtin_amdgcn_ballot_w64(mine)) {
        if (mine) {
            w.val = w.hit ? w.val + v : v;   // the first product is stored, later ones added (spgemm_row)
            w.hit = true;
        }
    } else if (APPEND) {
        if (w.m == kSpgemmMaxW) { err |= kRefillLong; return; }
        if (lane == w.m) { w.col = j; w.val = v; w.hit = true; }
        ++w.m;
    } else {
        err |= kRefillMissing;
    }
}

// The wide form's output row (mpbp_*_refill_wide): lane t holds entries t and t + 64 of a row of m <= kSpgemmWideW
// entries.  Its pattern is fixed (never APPEND), and an entry still receives its products one by one in the traversal's
// order, so the sums are WaveRow's.
struct WaveRow2 {
    int32_t col, col2;
    double val, val2;
    bool hit, hit2;
    int m;
};
// the product (j, v) added to the entry of column j; false on every lane when the row lacks that column
__device__ inline bool wave_take(WaveRow& w, int lane, int32_t j, double v) {
    const bool mine = lane < w.m && w.col == j;
    if (mine) {
        w.val = w.hit ? w.val + v : v;
        w.hit = true;
    }
    return mine;
}
__device__ inline bool wave_take(WaveRow2& w, int lane, int32_t j, double v) {
    const bool mine = lane < w.m && w.col == j, mine2 = lane + 64 < w.m && w.col2 == j;
    if (mine) {
        w.val = w.hit ? w.val + v : v;
        w.hit = true;
    }
    if (mine2) {
        w.val2 = w.hit2 ? w.val2 + v : v;
        w.hit2 = true;
    }
    return mine || mine2;
}
template <bool APPEND>
__device__ inline void wave_feed(WaveRow2& w, int lane, int32_t j, double v, int& err) {
    static_assert(!APPEND, "a wide row's pattern is fixed");
    if (!__builtin_amdgcn_ballot_w64(wave_take(w, lane, j, v))) err |= kRefillMissing;
}

__device__ inline int64_t lane_get(int64_t v, int src) {
    return ((int64_t)__builtin_amdgcn_readlane((int32_t)(v >> 32), src) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int32_t)v, src);
}

// inclusive prefix sum over the wave's lanes
__device__ inline int64_t wave_scan(int64_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// lane t's value sent to lane dst (a permutation of the lanes)
__device__ inline int32_t lane_push(int32_t v, int dst) { return __builtin_amdgcn_ds_permute(dst << 2, v); }
__device__ inline double lane_push(double v, int dst) {
    return __hiloint2double(lane_push(__double2hiint(v), dst), lane_push(__double2loint(v), dst));
}

// Feeds a_i * (row k_i of B) for the entries i < n the lanes hold (lane i: k, a), in entry order, each row in B's
// order: spgemm_row's traversal of one A row.  The rows' extents, then their entries 64 at a time, are loaded one per
// lane and the products formed there, so no row costs a dependent memory round trip of its own; only the accumulation
// walks the products one by one.
template <bool APPEND, class Row>
__device__ inline void wave_feed_rows(Row& w, int lane, int n, int32_t k, double a, const RCsr& B, int& err) {
    int32_t b0 = 0, len = 0;
    bool bad = false;
    if (lane < n) {
        bad = k < 0 || k >= B.nrows;
        if (!bad) {
            b0 = B.rp[k];
            const int32_t b1 = B.rp[k + 1];
            bad = b0 < 0 || b0 > b1 || (int64_t)b1 > B.nnz;
            if (!bad) len = b1 - b0;
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad)) { err |= kRefillIndex; return; }
    const int64_t incl = wave_scan(len, lane), excl = incl - len;   // products before / through entry `lane`
    const int64_t total = lane_get(incl, 63);
    int cur = 0;   // the first entry with products at or after `base`
    for (int64_t base = 0; base < total; base += 64) {
        const int64_t p = base + lane;   // this lane's product of the round
        while (cur < n && lane_get(incl, cur) <= base) ++cur;
        int own = -1;
        for (int i = cur; i < n && lane_get(excl, i) < base + 64; ++i)
            if (p >= lane_get(excl, i) && p < lane_get(incl, i)) own = i;
        const int src = own < 0 ? 0 : own;
        const int64_t at = (int64_t)__shfl(b0, src, 64) + (p - __shfl(excl, src, 64));
        const double aa = __shfl(a, src, 64);
        int32_t j = 0;
        double v = 0.0;
        if (own >= 0) { j = B.ci[at]; v = aa * B.va[at]; }
        const int cnt = (int)min((int64_t)64, total - base);
        for (int q = 0; q < cnt; ++q) wave_feed<APPEND>(w, lane, lane_get(j, q), lane_get(v, q), err);
    }
}

// row r of A B in spgemm_row's traversal order
template <bool APPEND, class Row>
__device__ inline void wave_feed_product(Row& w, int lane, const RCsr& A, const RCsr& B, int32_t r, int& err) {
    int32_t a0, a1;
    if (r < 0 || r >= A.nrows || !row_extent(A, r, a0, a1)) { err |= kRefillIndex; return; }
    for (int64_t ca = a0; ca < a1; ca += 64) {
        const int na = (int)min((int64_t)64, a1 - ca);
        int32_t ak = 0;
        double av = 0.0;
        if (lane < na) { ak = A.ci[ca + lane]; av = A.va[ca + lane]; }
        wave_feed_rows<APPEND>(w, lane, na, ak, av, B, err);
    }
}

// lane t's rank among the row's columns (they are distinct): entry `rank` of the sorted row; lanes past the row keep
// their own index, so the ranks are a permutation of the lanes
__device__ inline int wave_rank(const WaveRow& w, int lane) {
    int rank = 0;
    for (int u = 0; u < w.m; ++u) rank += lane_get(w.col, u) < w.col ? 1 : 0;
    return lane < w.m ? rank : lane;
}

constexpr int kRefillPair = 0, kRefillLeft = 1, kRefillRight = 2;

// MODE pair:  C = alpha_outer X Y                    (Z unused)
//      left:  C = alpha_outer (alpha_inner X Y) Z    -- inner row r once per output row, consumed in sorted-column
//             order (the order spgemm_fill stored it in)
//      right: C = alpha_outer X (alpha_inner Y Z)    -- inner row k per entry (r, k) of X; its columns are distinct,
//             so each goes to another output entry and their order within the row reaches no sum
//      WIDE:  output rows up to kSpgemmWideW entries, two per lane (WaveRow2); inner rows stay within a wave's 64
template <int MODE, bool WIDE = false>
__global__ void __launch_bounds__(kBlock) k_refill(RCsr X, RCsr Y, RCsr Z, double alpha_inner, double alpha_outer,
                                                   RCsr C, double* cva, int* errs) {
    const int lane = threadIdx.x & 63;
    const int32_t r = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
    if (r >= C.nrows) return;
    int err = 0;
    int32_t c0, c1;
    if (!row_extent(C, r, c0, c1)) err |= kRefillIndex;
    else if (c1 - c0 > (WIDE ? kSpgemmWideW : kSpgemmMaxW)) err |= WIDE ? kRefillWide : kRefillLong;
    if (!err) {
        typename std::conditional<WIDE, WaveRow2, WaveRow>::type w{};
        w.m = c1 - c0;
        if (lane < w.m) w.col = C.ci[c0 + lane];
        if constexpr (WIDE)
            if (lane + 64 < w.m) w.col2 = C.ci[c0 + 64 + lane];
        if (MODE == kRefillPair) {
            wave_feed_product<false>(w, lane, X, Y, r, err);
        } else if (MODE == kRefillLeft) {
            WaveRow t{0, 0.0, false, 0};
            wave_feed_product<true>(t, lane, X, Y, r, err);
            const int rank = wave_rank(t, lane);
            wave_feed_rows<false>(w, lane, t.m, lane_push(t.col, rank), lane_push(alpha_inner * t.val, rank), Z, err);
        } else {
            int32_t x0 = 0, x1 = 0;
            if (!row_extent(X, r, x0, x1)) { err |= kRefillIndex; x1 = x0 = 0; }
            for (int64_t cx = x0; cx < x1; cx += 64) {
                const int nx = (int)min((int64_t)64, x1 - cx);
                int32_t xk = 0;
                double xv = 0.0;
                if (lane < nx) { xk = X.ci[cx + lane]; xv = X.va[cx + lane]; }
                for (int i = 0; i < nx; ++i) {
                    WaveRow t{0, 0.0, false, 0};
                    wave_feed_product<true>(t, lane, Y, Z, lane_get(xk, i), err);
                    const double xt = lane_get(xv, i) * (alpha_inner * t.val);
                    bool got = false;
                    int taken = 0;   // WIDE: a lane may receive two of the inner row's products (its two entries)
                    for (int s = 0; s < t.m; ++s) {
                        const int32_t j = lane_get(t.col, s);
                        const double v = lane_get(xt, s);
                        if constexpr (WIDE) {
                            taken += __builtin_amdgcn_ballot_w64(wave_take(w, lane, j, v)) ? 1 : 0;
                        } else if (lane < w.m && w.col == j) {
                            w.val = w.hit ? w.val + v : v;
                            w.hit = got = true;
                        }
                    }
                    if constexpr (WIDE) {
                        if (taken != t.m) err |= kRefillMissing;
                    } else if (__popcll((unsigned long long)__builtin_amdgcn_ballot_w64(got)) != t.m) {
                        err |= kRefillMissing;
                    }
                }
            }
        }
        if (!err && lane < w.m) cva[c0 + lane] = w.hit ? alpha_outer * w.val : 0.0;
        if constexpr (WIDE)
            if (!err && lane + 64 < w.m) cva[c0 + 64 + lane] = w.hit2 ? alpha_outer * w.val2 : 0.0;
    }
    if (err && lane == 0) {
        atomicOr(&errs[0], err);
        atomicAdd(&errs[1], 1);
    }
}

// ============================================================ helpers ====
__global__ void k_csr_diag(Csr A, int32_t nrows, int32_t col_offset, double* diag, int* missing) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    double d = 0.0;
    bool found = false;
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k)
        if (A.ci[k] == r + col_offset) { d = A.va[k]; found = true; }
    diag[r] = d;
    if (!found) atomicAdd(missing, 1);
}

__global__ void k_gershgorin(Csr A, int32_t nrows, const double* diag, unsigned long long* out) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    double q = 0.0;
    if (r < nrows) {
        double s = 0.0;
        for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k) s += fabs(A.va[k]);
        q = s / fabs(diag[r]);
    }
    // non-negative doubles order like their bit patterns
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(q, d, 64);
        q = o > q ? o : q;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(q));
}

__global__ void k_extract_count(Csr A, const int32_t* rows, int32_t nloc, int32_t* row_nnz) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nloc) return;
    const int32_t r = rows[i];
    row_nnz[i] = A.rp[r + 1] - A.rp[r];
}

__global__ void k_extract_fill(Csr A, const int32_t* rows, int32_t nloc, const int32_t* colmap,
                               const int32_t* lrp, int32_t* lci, double* lva, int* bad) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nloc) return;
    const int32_t r = rows[i];
    int32_t o = lrp[i];
    for (int32_t k = A.rp[r]; k < A.rp[r + 1]; ++k, ++o) {   // keep the global row's order
        const int32_t lc = colmap[A.ci[k]];
        if (lc < 0) atomicAdd(bad, 1);
        lci[o] = lc < 0 ? 0 : lc;
        lva[o] = A.va[k];
    }
}

__global__ void k_gather(int32_t count, const int32_t* idx, const double* src, double* dst) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = src[idx[i]];
}

__global__ void k_scatter(int32_t count, const int32_t* idx, const double* src, double* dst) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[idx[i]] = src[i];
}

// ============================================================ multigrid transfers ====
// Geometric coarsening of a periodic n x n MAC grid by 2 in each direction, field by field.  Along an axis a
// field is cell-centred (MPBP_MG_CELL: fine 2i and 2i+1 lie around coarse i, linear weights 3/4, 1/4) or
// node-centred (MPBP_MG_NODE: fine 2i sits on coarse i, fine 2i+1 halfway to coarse i+1).  P (fine <- coarse)
// is the tensor product of the two 1D lists; R = P^T exactly.  Every weight is a dyadic rational, so the
// values are exact and the columns of each row come out sorted (periodic wrap included).
struct MgFields {
    int32_t nfields;
    int32_t ky[8], kx[8];
};

template <int CAP>
__device__ inline void sort_pairs(int m, int* idx, double* w) {
#pragma unroll
    for (int a = 1; a < CAP; ++a)
#pragma unroll
        for (int b = CAP - 1; b >= a; --b)
            if (b < m && idx[b - 1] > idx[b]) {
                const int ti = idx[b - 1];
                idx[b - 1] = idx[b];
                idx[b] = ti;
                const double tw = w[b - 1];
                w[b - 1] = w[b];
                w[b] = tw;
            }
}

// P's 1D list for fine index f (coarse size nc): <= 2 entries.
__device__ inline int mg_p1d(int kind, int nc, int f, int* idx, double* w) {
    const int i = f >> 1;
    if (kind == MPBP_MG_NODE && !(f & 1)) {
        idx[0] = i;
        w[0] = 1.0;
        return 1;
    }
    const int j = (kind == MPBP_MG_CELL && !(f & 1)) ? (i + nc - 1) % nc : (i + 1) % nc;
    idx[0] = i;
    w[0] = kind == MPBP_MG_CELL ? 0.75 : 0.5;
    idx[1] = j;
    w[1] = kind == MPBP_MG_CELL ? 0.25 : 0.5;
    sort_pairs<2>(2, idx, w);
    return 2;
}

// R's 1D list for coarse index i (fine size nf) = column i of P: <= 4 entries.
__device__ inline int mg_r1d(int kind, int nf, int i, int* idx, double* w) {
    const int f = 2 * i;
    int m;
    if (kind == MPBP_MG_CELL) {
        idx[0] = (f + nf - 1) % nf; w[0] = 0.25;
        idx[1] = f;                 w[1] = 0.75;
        idx[2] = f + 1;             w[2] = 0.75;
        idx[3] = (f + 2) % nf;      w[3] = 0.25;
        m = 4;
    } else {
        idx[0] = (f + nf - 1) % nf; w[0] = 0.5;
        idx[1] = f;                 w[1] = 1.0;
        idx[2] = f + 1;             w[2] = 0.5;
        m = 3;
    }
    sort_pairs<4>(m, idx, w);
    return m;
}

// Unsigned division by a run-time invariant d (>= 1) with one high multiply (Granlund-Montgomery, round-up variant):
// q = (umulhi(x, m) + x) >> s for every 32-bit x.
struct DivU {
    uint32_t m, s;
};
inline DivU divu(uint32_t d) {
    uint32_t s = 0;
    while ((uint64_t(1) << s) < d) ++s;
    const uint64_t m = ((uint64_t(1) << 32) * ((uint64_t(1) << s) - d)) / d + 1;
    return DivU{(uint32_t)m, s};
}
__device__ inline uint32_t divu(uint32_t x, DivU d) {
    return (uint32_t)(((uint64_t)__umulhi(x, d.m) + x) >> d.s);
}

// P's 1D list for fine index f (coarse size nc), in increasing index order (= mg_p1d's sorted list)
__device__ inline int mg_p1d_fast(int kind, int nc, int f, int* idx, double* w) {
    const int i = f >> 1;
    if (kind == MPBP_MG_NODE && !(f & 1)) {
        idx[0] = i;
        w[0] = 1.0;
        return 1;
    }
    const double wi = kind == MPBP_MG_CELL ? 0.75 : 0.5, wj = kind == MPBP_MG_CELL ? 0.25 : 0.5;
    const bool down = kind == MPBP_MG_CELL && !(f & 1);             // the other coarse point is i - 1, else i + 1
    const int j = down ? (i == 0 ? nc - 1 : i - 1) : (i + 1 == nc ? 0 : i + 1);
    const bool jfirst = j < i;
    idx[0] = jfirst ? j : i;  w[0] = jfirst ? wj : wi;
    idx[1] = jfirst ? i : j;  w[1] = jfirst ? wi : wj;
    return 2;
}
// R's 1D list for coarse index i (fine size nf), in increasing index order (= mg_r1d's sorted list)
__device__ inline int mg_r1d_fast(int kind, int nf, int i, int* idx, double* w) {
    const int f = 2 * i;
    if (kind == MPBP_MG_CELL) {   // f-1, f, f+1, f+2 with 1/4, 3/4, 3/4, 1/4; the wrapped one moves to its end
        if (f == 0) {
            idx[0] = 0; w[0] = 0.75; idx[1] = 1; w[1] = 0.75; idx[2] = 2 % nf; w[2] = 0.25; idx[3] = nf - 1; w[3] = 0.25;
        } else if (f + 2 == nf) {
            idx[0] = 0; w[0] = 0.25; idx[1] = f - 1; w[1] = 0.25; idx[2] = f; w[2] = 0.75; idx[3] = f + 1; w[3] = 0.75;
        } else {
            idx[0] = f - 1; w[0] = 0.25; idx[1] = f; w[1] = 0.75; idx[2] = f + 1; w[2] = 0.75; idx[3] = f + 2; w[3] = 0.25;
        }
        return 4;
    }
    if (f == 0) {                 // f-1, f, f+1 with 1/2, 1, 1/2
        idx[0] = 0; w[0] = 1.0; idx[1] = 1; w[1] = 0.5; idx[2] = nf - 1; w[2] = 0.5;
    } else {
        idx[0] = f - 1; w[0] = 0.5; idx[1] = f; w[1] = 1.0; idx[2] = f + 1; w[2] = 0.5;
    }
    return 3;
}

// y = op(T x) for T = P or R of the n x n grid (n = fine size), matrix-free: each row rebuilds its tensor-product
// weights and columns exactly as k_mg_transfer stores them (same order, same products), so the sums are the CSR
// SpMV's bit for bit; no matrix stream, and the x gathers issue without waiting for column loads.  The row's field
// and grid position come from two multiply-shift divisions and the 1D lists from selects (no integer division, no
// sorting network: 28 -> ~8 us for the 1024^2 prolongation).
struct MgDiv {
    DivU per, nr;   // rows per field, grid size of the rows' level
};
// Row `row` of T = P (rows = fine unknowns) or R (rows = coarse unknowns) of the n x n fine grid: its field, the 1D
// lists of both directions and the columns' field offset (nk = the columns' grid size).  The one place the matrix-free
// transfers build a row, so every kernel that folds a transfer in takes the same lists in the same order.
struct MgRow {
    int my, mx, nk, off;
    int yi[4], xi[4];
    double yw[4], xw[4];
};
__device__ inline void mg_row(const MgFields& F, const MgDiv& dv, int32_t n, int32_t which, int32_t row, MgRow& T) {
    const int nc = n / 2;
    const int nr = which == MPBP_MG_P ? n : nc;
    T.nk = which == MPBP_MG_P ? nc : n;
    const uint32_t per = (uint32_t)nr * (uint32_t)nr;
    const int fld = (int)divu((uint32_t)row, dv.per);
    const uint32_t cell = (uint32_t)row - (uint32_t)fld * per;
    const int r = (int)divu(cell, dv.nr), c = (int)(cell - (uint32_t)r * (uint32_t)nr);
    T.my = which == MPBP_MG_P ? mg_p1d_fast(F.ky[fld], nc, r, T.yi, T.yw) : mg_r1d_fast(F.ky[fld], n, r, T.yi, T.yw);
    T.mx = which == MPBP_MG_P ? mg_p1d_fast(F.kx[fld], nc, c, T.xi, T.xw) : mg_r1d_fast(F.kx[fld], n, c, T.xi, T.xw);
    T.off = fld * T.nk * T.nk;
}
template <class Epi>
__global__ void __launch_bounds__(kBlock) k_mg_transfer_spmv(MgFields F, MgDiv dv, int32_t n, int32_t which,
                                                             int32_t nrows, const double* __restrict__ x, Epi epi) {
    const int32_t row = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (row >= nrows) return;
    const typename Epi::P pe = epi.pre(row);
    MgRow T;
    mg_row(F, dv, n, which, row, T);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)   // (constant trip counts keep the lists in registers)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (a < T.my && b < T.mx) acc += (T.yw[a] * T.xw[b]) * x[T.off + T.yi[a] * T.nk + T.xi[b]];
    epi(row, acc, pe);
}

// which: MPBP_MG_P (rows = fine unknowns) or MPBP_MG_R (rows = coarse unknowns); n = fine grid size.
// rl (optional): the global rows to build, output row i = rl[i] (a rank's band of a row-partitioned hierarchy)
__global__ void k_mg_transfer(MgFields F, int32_t n, int32_t which, int64_t nrows, const int32_t* rp,
                              int32_t* row_nnz, int32_t* ci, double* va, const int32_t* rl = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const int64_t row = rl ? (int64_t)rl[i] : i;
    const int nc = n / 2;
    const int nr = which == MPBP_MG_P ? n : nc;       // grid size of the rows' level
    const int nk = which == MPBP_MG_P ? nc : n;       // ... and of the columns' level
    const int64_t per = (int64_t)nr * nr;
    const int fld = (int)(row / per);
    const int64_t cell = row - fld * per;
    const int r = (int)(cell / nr), c = (int)(cell % nr);
    int yi[4], xi[4];
    double yw[4], xw[4];
    const int my = which == MPBP_MG_P ? mg_p1d(F.ky[fld], nc, r, yi, yw) : mg_r1d(F.ky[fld], n, r, yi, yw);
    const int mx = which == MPBP_MG_P ? mg_p1d(F.kx[fld], nc, c, xi, xw) : mg_r1d(F.kx[fld], n, c, xi, xw);
    if (row_nnz) {
        row_nnz[i] = my * mx;
        return;
    }
    const int64_t off = (int64_t)fld * nk * nk;
    int32_t k = rp[i];
    for (int a = 0; a < my; ++a)
        for (int b = 0; b < mx; ++b) {
            ci[k] = (int32_t)(off + (int64_t)yi[a] * nk + xi[b]);
            va[k] = yw[a] * xw[b];
            ++k;
        }
}

// ---- coarsening of any fine size (mpbp_mg_transfer_any_*, Multigrid(coarsen="any")) ----
// Fine size nf >= 5 (odd or even) coarsens to nc = nf / 2 (floor).  Fine point f sits at the coarse coordinate
// t_f = num / den, from integers only -- node-centred: num = f nc, den = nf; cell-centred: num = (2 f + 1) nc - nf,
// den = 2 nf (negative at f = 0: the floor is towards -inf) -- and is interpolated linearly from the coarse points
// i0 = floor(t_f) and i0 + 1 on the periodic grid: weights (den - rem) / den and rem / den with rem = num - i0 den, each
// ONE division of two exactly representable integers (never 1 - w), a single entry of weight 1.0 when rem == 0.  For even
// nf these are mg_p1d's lists, indices and bits.  R = P^T takes the same quotients: coarse i collects the (unwrapped)
// fine points with |num - i den| < den, at most 5 of them, distinct modulo nf since nf >= 5.
// I: int64_t (the stored builders) or int32_t (the matrix-free rows: nf <= kMgAnyMaxN keeps every product below 2^31).
constexpr int kMgAnyMaxN = 32768;
template <class I>
__device__ inline I mg_floor_div(I a, I b) {   // b > 0
    const I q = a / b;
    return (a - q * b) < 0 ? q - 1 : q;
}
template <class I>
__device__ inline I mg_any_num(int kind, I nf, I nc, I f) {
    return kind == MPBP_MG_NODE ? f * nc : (2 * f + 1) * nc - nf;
}
// P's 1D list for fine index f (fine size nf): 1 or 2 entries, in increasing index order
template <class I>
__device__ inline int mg_p1d_any(int kind, int nf_, int f, int* idx, double* w) {
    const I nf = nf_, nc = nf_ / 2, den = kind == MPBP_MG_NODE ? nf : 2 * nf;
    const I num = mg_any_num<I>(kind, nf, nc, (I)f);
    const I i0 = mg_floor_div<I>(num, den), rem = num - i0 * den;
    I a = i0 % nc;
    if (a < 0) a += nc;
    if (rem == 0) {
        idx[0] = (int)a;
        w[0] = 1.0;
        return 1;
    }
    const I b = a + 1 == nc ? 0 : a + 1;
    const double wa = (double)(den - rem) / (double)den, wb = (double)rem / (double)den;
    const bool bfirst = b < a;
    idx[0] = (int)(bfirst ? b : a);  w[0] = bfirst ? wb : wa;
    idx[1] = (int)(bfirst ? a : b);  w[1] = bfirst ? wa : wb;
    return 2;
}
// R's 1D list for coarse index i (fine size nf) = column i of P: 3 to 5 entries, in increasing index order
template <class I>
__device__ inline int mg_r1d_any(int kind, int nf_, int i, int* idx, double* w) {
    const I nf = nf_, nc = nf_ / 2, den = kind == MPBP_MG_NODE ? nf : 2 * nf;
    // the first fine index with num > (i - 1) den -- node: f nc > (i - 1) nf; cell: (2 f + 1) nc > (2 i - 1) nf -- is one
    // past the floor of the bound; the window's members follow it consecutively (num grows with f), in [-3, nf + 3)
    const I f0 = 1 + (kind == MPBP_MG_NODE ? mg_floor_div<I>(((I)i - 1) * nf, nc)
                                           : mg_floor_div<I>((2 * (I)i - 1) * nf - nc, 2 * nc));
    int m = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {   // (constant indices keep the lists in registers)
        const I f = f0 + j;
        const I val = mg_any_num<I>(kind, nf, nc, f) - (I)i * den;   // (t_f - i) den > -den
        const bool in = val < den;
        idx[j] = (int)(f < 0 ? f + nf : f >= nf ? f - nf : f);
        w[j] = (double)(val < 0 ? den + val : den - val) / (double)den;
        m += in ? 1 : 0;
    }
    sort_pairs<5>(m, idx, w);
    return m;
}

struct MgRowAny {
    int my, mx, nk, off;
    int yi[5], xi[5];
    double yw[5], xw[5];
};
// y = op(T x) for the any-size P or R, matrix-free: each row rebuilds mg_p1d_any / mg_r1d_any's lists, the products
// and the order k_mg_transfer_any stores, so the sums are the stored CSR's SpMV bit for bit (as k_mg_transfer_spmv
// is to k_mg_transfer).  n <= kMgAnyMaxN.
template <class Epi>
__global__ void __launch_bounds__(kBlock) k_mg_transfer_any_spmv(MgFields F, MgDiv dv, int32_t n, int32_t which,
                                                                 int32_t nrows, const double* __restrict__ x, Epi epi) {
    const int32_t row = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (row >= nrows) return;
    const typename Epi::P pe = epi.pre(row);
    const int nc = n / 2;
    const int nr = which == MPBP_MG_P ? n : nc, nk = which == MPBP_MG_P ? nc : n;
    const uint32_t per = (uint32_t)nr * (uint32_t)nr;
    const int fld = (int)divu((uint32_t)row, dv.per);
    const uint32_t cell = (uint32_t)row - (uint32_t)fld * per;
    const int r = (int)divu(cell, dv.nr), c = (int)(cell - (uint32_t)r * (uint32_t)nr);
    MgRowAny T;
    T.my = which == MPBP_MG_P ? mg_p1d_any<int32_t>(F.ky[fld], n, r, T.yi, T.yw) : mg_r1d_any<int32_t>(F.ky[fld], n, r, T.yi, T.yw);
    T.mx = which == MPBP_MG_P ? mg_p1d_any<int32_t>(F.kx[fld], n, c, T.xi, T.xw) : mg_r1d_any<int32_t>(F.kx[fld], n, c, T.xi, T.xw);
    const int off = fld * nk * nk;
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a)   // (constant trip counts keep the lists in registers)
#pragma unroll
        for (int b = 0; b < 5; ++b)
            if (a < T.my && b < T.mx) acc += (T.yw[a] * T.xw[b]) * x[off + T.yi[a] * nk + T.xi[b]];
    epi(row, acc, pe);
}

// The stored form: rows of P (which = MPBP_MG_P, rows = fine unknowns) or R = P^T (rows = coarse unknowns) of the
// n x n fine grid, n >= 5; row_nnz set: count only.
__global__ void k_mg_transfer_any(MgFields F, int32_t n, int32_t which, int64_t nrows, const int32_t* rp,
                                  int32_t* row_nnz, int32_t* ci, double* va) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    const int nc = n / 2;
    const int nr = which == MPBP_MG_P ? n : nc;       // grid size of the rows' level
    const int nk = which == MPBP_MG_P ? nc : n;       // ... and of the columns' level
    const int64_t per = (int64_t)nr * nr;
    const int fld = (int)(row / per);
    const int64_t cell = row - fld * per;
    const int r = (int)(cell / nr), c = (int)(cell % nr);
    int yi[5], xi[5];
    double yw[5], xw[5];
    const int my = which == MPBP_MG_P ? mg_p1d_any<int64_t>(F.ky[fld], n, r, yi, yw) : mg_r1d_any<int64_t>(F.ky[fld], n, r, yi, yw);
    const int mx = which == MPBP_MG_P ? mg_p1d_any<int64_t>(F.kx[fld], n, c, xi, xw) : mg_r1d_any<int64_t>(F.kx[fld], n, c, xi, xw);
    if (row_nnz) {
        row_nnz[row] = my * mx;
        return;
    }
    const int64_t off = (int64_t)fld * nk * nk;
    int32_t k = rp[row];
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            if (a < my && b < mx) {
                ci[k] = (int32_t)(off + (int64_t)yi[a] * nk + xi[b]);
                va[k] = yw[a] * xw[b];
                ++k;
            }
}

// ================================================================== SpMV ====
// Row blocks are dealt round-robin over the 8 XCDs; give every XCD a contiguous run of
// blocks instead, so the +-n stencil neighbours of a block's rows sit in the same L2.
// Placement changes speed only, never results.
__device__ inline int xcd_swizzle(int b, int nb) {
    const int full = nb & ~7;
    if (b >= full) return b;
    const int per = full >> 3;
    return (b & 7) * per + (b >> 3);
}

// Epilogues.  pre(r) issues the row's operand loads at kernel start (they overlap the matrix
// stream); operator() finishes the row once its sum is known.
struct EpiStore {
    double* y;
    struct P {};
    __device__ P pre(int32_t) const { return {}; }
    __device__ P pre_lite(int32_t) const { return {}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P&) const { st_stream<NT>(y + r, acc); }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
struct EpiAdd {   // rhs = D Finv_v + v_p   (solve.py:259)
    const double* z;
    double* y;
    struct P { double z; };
    __device__ P pre(int32_t r) const { return {ld_stream(z + r)}; }
    __device__ P pre_lite(int32_t r) const { return {ld_stream(z + r)}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const { st_stream<NT>(y + r, acc + p.z); }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
// The pressure solves' right-hand sides, written with the first Gt_G sweep's staged iterate beside them:
// y = rhs and x0 = c2 (rhs / diag) -- the value that sweep would otherwise recompute at each staged point (XInit),
// so the sweep stages x0 from memory (same bits).  EpiAddX0: rhs = D Finv_v + v_p (solve.py:259); EpiStoreX0:
// x_b = Gt_F_G x_a (solve.py:267).
struct EpiAddX0 {
    const double* z;
    double* y;
    const double* diag;
    double c2;
    double* x0;
    struct P { double z, pdiag; };
    __device__ P pre(int32_t r) const { return {ld_stream(z + r), diag[r]}; }
    __device__ P pre_lite(int32_t r) const { return pre(r); }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const {
        const double v = acc + p.z;
        st_stream<NT>(y + r, v);
        st_stream<NT>(x0 + r, c2 * (v / p.pdiag));
    }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
struct EpiStoreX0 {
    double* y;
    const double* diag;
    double c2;
    double* x0;
    struct P { double pdiag; };
    __device__ P pre(int32_t r) const { return {diag[r]}; }
    __device__ P pre_lite(int32_t r) const { return pre(r); }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const {
        st_stream<NT>(y + r, acc);
        st_stream<NT>(x0 + r, c2 * (acc / p.pdiag));
    }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
struct EpiResid {
    const double* z;
    double* y;
    struct P { double z; };
    __device__ P pre(int32_t r) const { return {ld_stream(z + r)}; }
    __device__ P pre_lite(int32_t r) const { return {ld_stream(z + r)}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const { st_stream<NT>(y + r, p.z - acc); }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
// EpiAdd / EpiResid with z loaded once the row's sum is known instead of ahead of it (pre requests nothing): the
// five-row A policy (StokesADev) has no registers left to hold five z values through its rows at k_march's 4 waves
// per SIMD -- with EpiAdd / EpiResid its instances spilled 24-72 B per lane.  Same operation, same bits.
struct EpiAddLate {
    const double* z;
    double* y;
    struct P {};
    __device__ P pre(int32_t) const { return {}; }
    __device__ P pre_lite(int32_t) const { return {}; }
    __device__ void operator()(int32_t r, double acc, const P&) const { y[r] = acc + ld_stream(z + r); }
};
struct EpiResidLate {
    const double* z;
    double* y;
    struct P {};
    __device__ P pre(int32_t) const { return {}; }
    __device__ P pre_lite(int32_t) const { return {}; }
    __device__ void operator()(int32_t r, double acc, const P&) const { y[r] = ld_stream(z + r) - acc; }
};
// The solver epilogues carry two run-time switches -- `sub` (the solve's last sweep returns sub - x) and
// `store_d` (the direction is stored except on a solve's last sweep).  The marching kernels get them as
// template flags instead (FIXED = true; launch_march picks the instance): no load or store then sits under
// a branch (the compiler's wait counts stay exact) and the unused operand costs no registers.
// RCP (tolerance-mode F policy only, FStencilFast): the diagonal handed over by set_diag is its reciprocal, so the
// update multiplies instead of dividing.
template <bool FIXED = false, bool SUB = true, bool RCP = false>
struct EpiJacobiT {   // x = (b - R x)/D in residual form (solve.py:158)
    const double* xin;
    const double* b;
    const double* diag;
    const double* sub;
    double* xout;
    struct P { double x, b, dg, s; };
    __device__ bool has_sub() const { return FIXED ? SUB : sub != nullptr; }
    __device__ P pre(int32_t r) const { return {xin[r], ld_stream(b + r), diag ? diag[r] : 0.0, sub ? ld_stream(sub + r) : 0.0}; }
    // x_in and diag supplied by the caller (set_x / set_diag)
    __device__ P pre_lite(int32_t r) const { return {0.0, ld_stream(b + r), 0.0, has_sub() ? ld_stream(sub + r) : 0.0}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const {
        const double x = p.x + (RCP ? (p.b - acc) * p.dg : (p.b - acc) / p.dg);
        st_stream<NT>(xout + r, has_sub() ? p.s - x : x);
    }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
// BX (FIXED instances of the marching kernels only): b is not loaded -- the kernel recomputes it per row and hands
// it over with set_b (the second F solve's right-hand side W = G x_p, solve.py:273-274, never stored).
template <bool FIXED = false, bool SUB = true, bool SD = true, bool BX = false, bool RCP = false>
struct EpiChebT {
    const double* xin;
    const double* b;
    const double* diag;
    double* d;
    double c1, c2;
    const double* sub;
    double* xout;
    int store_d = 1;   // 0: the inner solve's last sweep (its direction is never read again)
    struct P { double x, b, dg, d, s; };
    __device__ bool has_sub() const { return FIXED ? SUB : sub != nullptr; }
    __device__ bool stores_d() const { return FIXED ? SD : store_d != 0; }
    __device__ P pre(int32_t r) const { return {xin[r], ld_stream(b + r), diag ? diag[r] : 0.0, ld_stream(d + r), sub ? ld_stream(sub + r) : 0.0}; }
    // BX: `sub` is loaded in the epilogue itself instead of ahead of the row -- the fused
    // second solve's last sweep otherwise spills (128 VGPRs + 24 B scratch): 40.9 -> 38.9 us per launch
    // (2541-2565 -> 2573-2640 applies/s, A/B on one box)
    static constexpr bool kSubLate = BX, kBX = BX;
    __device__ P pre_lite(int32_t r) const { return {0.0, BX ? 0.0 : ld_stream(b + r), 0.0, ld_stream(d + r), (has_sub() && !kSubLate) ? ld_stream(sub + r) : 0.0}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const {
        const double z = RCP ? (p.b - acc) * p.dg : (p.b - acc) / p.dg;
        const double dn = c1 * p.d + c2 * z;
        if (stores_d()) st_stream<NT>(d + r, dn);
        const double x = p.x + dn;
        const double sv = kSubLate && has_sub() ? ld_stream(sub + r) : p.s;
        st_stream<NT>(xout + r, has_sub() ? sv - x : x);
    }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
// EpiCheb for the first sweep after x0 = d0 = c2[0] b / diag: the previous direction is the staged x0
// itself (x and diag supplied by the stencil via set_x / set_diag), so d is written but not read.
template <bool FIXED = false, bool SUB = true, bool SD = true, bool BX = false, bool RCP = false>
struct EpiChebFirstT {
    const double* b;
    double* d;
    double c1, c2;
    const double* sub;
    double* xout;
    int store_d = 1;
    struct P { double x, b, dg, s; };
    __device__ bool has_sub() const { return FIXED ? SUB : sub != nullptr; }
    __device__ bool stores_d() const { return FIXED ? SD : store_d != 0; }
    __device__ P pre(int32_t r) const { return {0.0, ld_stream(b + r), 0.0, sub ? ld_stream(sub + r) : 0.0}; }
    __device__ P pre_lite(int32_t r) const { return {0.0, BX ? 0.0 : ld_stream(b + r), 0.0, has_sub() ? ld_stream(sub + r) : 0.0}; }
    template <bool NT = false>
    __device__ void apply(int32_t r, double acc, const P& p) const {
        const double z = RCP ? (p.b - acc) * p.dg : (p.b - acc) / p.dg;
        const double dn = c1 * p.x + c2 * z;
        if (stores_d()) st_stream<NT>(d + r, dn);
        const double x = p.x + dn;
        st_stream<NT>(xout + r, has_sub() ? p.s - x : x);
    }
    __device__ void operator()(int32_t r, double acc, const P& p) const { apply<false>(r, acc, p); }
};
using EpiJacobi = EpiJacobiT<>;
using EpiCheb = EpiChebT<>;
using EpiChebFirst = EpiChebFirstT<>;

// Run fn with the epilogue's run-time switches turned into template flags (other epilogues unchanged).  RCP: the
// stencil hands over the reciprocal diagonal (FStencilFast), the solver epilogues multiply by it.
template <bool RCP = false, class Epi, class Fn>
__host__ inline int with_fixed_epi(const Epi& e, Fn&& fn) { return fn(e); }
template <bool RCP = false, class Fn>
__host__ inline int with_fixed_epi(const EpiJacobi& e, Fn&& fn) {
    return e.sub ? fn(EpiJacobiT<true, true, RCP>{e.xin, e.b, e.diag, e.sub, e.xout})
                 : fn(EpiJacobiT<true, false, RCP>{e.xin, e.b, e.diag, e.sub, e.xout});
}
template <bool RCP = false, class Fn>
__host__ inline int with_fixed_epi(const EpiCheb& e, Fn&& fn) {
#define MPBP_CHEB(SUB, SD) fn(EpiChebT<true, SUB, SD, false, RCP>{e.xin, e.b, e.diag, e.d, e.c1, e.c2, e.sub, e.xout, e.store_d})
    return e.sub ? (e.store_d ? MPBP_CHEB(true, true) : MPBP_CHEB(true, false))
                 : (e.store_d ? MPBP_CHEB(false, true) : MPBP_CHEB(false, false));
#undef MPBP_CHEB
}
template <bool RCP = false, class Fn>
__host__ inline int with_fixed_epi(const EpiChebFirst& e, Fn&& fn) {
#define MPBP_CHEBF(SUB, SD) fn(EpiChebFirstT<true, SUB, SD, false, RCP>{e.b, e.d, e.c1, e.c2, e.sub, e.xout, e.store_d})
    return e.sub ? (e.store_d ? MPBP_CHEBF(true, true) : MPBP_CHEBF(true, false))
                 : (e.store_d ? MPBP_CHEBF(false, true) : MPBP_CHEBF(false, false));
#undef MPBP_CHEBF
}

// The same, with b supplied by the kernel (BX): the F sweeps of the second F solve with W = G x_p recomputed.
template <bool RCP = false, class Epi, class Fn>
__host__ inline int with_fixed_epi_bx(const Epi& e, Fn&& fn) { return set_error(MPBP_ERR_ARG, "no BX epilogue"); }
template <bool RCP = false, class Fn>
__host__ inline int with_fixed_epi_bx(const EpiCheb& e, Fn&& fn) {
#define MPBP_CHEB(SUB, SD) fn(EpiChebT<true, SUB, SD, true, RCP>{e.xin, e.b, e.diag, e.d, e.c1, e.c2, e.sub, e.xout, e.store_d})
    return e.sub ? (e.store_d ? MPBP_CHEB(true, true) : MPBP_CHEB(true, false))
                 : (e.store_d ? MPBP_CHEB(false, true) : MPBP_CHEB(false, false));
#undef MPBP_CHEB
}
template <bool RCP = false, class Fn>
__host__ inline int with_fixed_epi_bx(const EpiChebFirst& e, Fn&& fn) {
#define MPBP_CHEBF(SUB, SD) fn(EpiChebFirstT<true, SUB, SD, true, RCP>{e.b, e.d, e.c1, e.c2, e.sub, e.xout, e.store_d})
    return e.sub ? (e.store_d ? MPBP_CHEBF(true, true) : MPBP_CHEBF(true, false))
                 : (e.store_d ? MPBP_CHEBF(false, true) : MPBP_CHEBF(false, false));
#undef MPBP_CHEBF
}

// Epilogues a tolerance-mode policy may feed: those that ignore the diagonal, and the RCP solver epilogues.
template <class E> struct RcpOk : std::false_type {};
template <> struct RcpOk<EpiStore> : std::true_type {};
template <> struct RcpOk<EpiAdd> : std::true_type {};
template <> struct RcpOk<EpiResid> : std::true_type {};
template <> struct RcpOk<EpiAddLate> : std::true_type {};
template <> struct RcpOk<EpiResidLate> : std::true_type {};
template <bool S> struct RcpOk<EpiJacobiT<true, S, true>> : std::true_type {};
template <bool S, bool D, bool B> struct RcpOk<EpiChebT<true, S, D, B, true>> : std::true_type {};
template <bool S, bool D, bool B> struct RcpOk<EpiChebFirstT<true, S, D, B, true>> : std::true_type {};

// A cell-wise epilogue (Epi::kCell; EpiCplChebT, mg_coupled.inc) finishes the NOUT rows of a cell together:
// cell(rows, sums, x, pre) instead of one operator() per row.  k_march and k_direct take it by an if constexpr branch.
template <class E, class = void> struct CellEpi : std::false_type {};
template <class E> struct CellEpi<E, std::enable_if_t<E::kCell>> : std::true_type {};

// XI entry xi * a * (1 - a) as the assembly evaluates it (left to right).
__device__ inline double xi_of(double xi, double a) { return xi * a * (1.0 - a); }

template <class PT>
__device__ inline void set_b(PT& p, double b) { p.b = b; }
template <class PT>
__device__ inline void set_diag(PT& p, double d) { p.dg = d; }
template <class PT>
__device__ inline void set_x(PT& p, double x) { p.x = x; }
template <>
__device__ inline void set_x<EpiStore::P>(EpiStore::P&, double) {}
template <>
__device__ inline void set_x<EpiAdd::P>(EpiAdd::P&, double) {}
template <>
__device__ inline void set_x<EpiResid::P>(EpiResid::P&, double) {}
template <>
__device__ inline void set_diag<EpiStore::P>(EpiStore::P&, double) {}
template <>
__device__ inline void set_diag<EpiAdd::P>(EpiAdd::P&, double) {}
template <>
__device__ inline void set_diag<EpiResid::P>(EpiResid::P&, double) {}
template <>
__device__ inline void set_x<EpiAddX0::P>(EpiAddX0::P&, double) {}
template <>
__device__ inline void set_diag<EpiAddX0::P>(EpiAddX0::P&, double) {}
template <>
__device__ inline void set_x<EpiAddLate::P>(EpiAddLate::P&, double) {}
template <>
__device__ inline void set_diag<EpiAddLate::P>(EpiAddLate::P&, double) {}
template <>
__device__ inline void set_x<EpiResidLate::P>(EpiResidLate::P&, double) {}
template <>
__device__ inline void set_diag<EpiResidLate::P>(EpiResidLate::P&, double) {}

// CSR SpMV over the same row blocks, one wavefront per 64-row quarter of a block and no block-wide
// barrier.  Each wave streams its rows' [row_ptr[ra], row_ptr[rb]) entries in chunks of kWaveCap with
// 16-byte loads (1 KiB of values per wave-instruction) and transposes the chunk through its own LDS
// (values and columns as pairs, 9 KiB); each lane then walks the part of its own row that lies in the
// chunk, gathers x for it and adds the products left to right, chunk after chunk -- the oracle's
// sequential order, so bit-exact.  Gathering per row (lane = row, as in SELL) makes one
// wave-instruction's x addresses the same stencil neighbour of 64 consecutive rows instead of all
// neighbours of ~10 rows: fewer cache lines per instruction (153 vs 172 us for the 1024^2 A).  A 1024^2
// A row block (12 entries per velocity row) is one chunk per wave.
// Measured dead end: no staging at all, each lane loading its own row (16-byte loads 96 B apart across
// the wave) -- 567 us, the texture addresser then touches ~48 cache lines per wave-instruction.
constexpr int kWaveCap = 768;                 // entries per wave chunk (64 rows x 12 entries)
constexpr int kWavePairs = kWaveCap / 128;     // 16-byte loads per lane per chunk
constexpr int kRowBatch = 8;                   // pairs of a row gathered at once (16 entries)

// A wave-uniform int32 element through a scalar (constant address space) load.
typedef __attribute__((address_space(4))) const int32_t cint32;
__device__ inline int32_t ld_uniform_i32(const int32_t* p, int32_t i) {
    return ((cint32*)p)[__builtin_amdgcn_readfirstlane(i)];
}

// Lanes of one wave exchange data through LDS: order the LDS writes before the reads (compiler
// and wave scope; a wave's LDS operations complete in order).
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave whose 64 rows all hold LEN entries (stencil operators: A's velocity rows 12, pressure rows 8,
// F's rows 10) from an even start: its entries are exactly one chunk, lane l's row is pairs
// [l*LEN/2, (l+1)*LEN/2) of it, so the loads, LDS transposition, gathers and sums unroll with no
// per-entry bounds tests.  Same additions in the same order as the general loop (bit-exact).
// XB: x gathered with buffer loads (one descriptor for x, a 32-bit byte offset per entry: no 64-bit
// address arithmetic per gather); needs ncols * 8 < 2^31.
// Returns false (nothing stored) when some row of the wave does not hold LEN entries.  The
// matrix loads are issued before that check -- they depend on the wave's first entry s alone (and stay inside
// [s, s + 64 LEN) = the wave's entries), so their HBM latency overlaps the per-row row_ptr loads' instead of
// following it.
// TRUST: the wave table says the wave is uniform (no row check).
// GL (table-trusted waves whose entry offset is a multiple of 4): the chunk is copied into LDS by LDS-DMA
// (global_load_lds_dwordx4, nontemporal) instead of through VGPRs -- the same lane-linear image, no staging registers
// or LDS stores: 137.0-137.3 vs 138.8-141.8 us for the 1024^2 A on one box (tools/spmv_lab.py, r05h).
__device__ inline void glds16(const void* g, void* lds) {
    __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)lds, 16, 0, 2);
}
template <int LEN, bool XB, class Epi, bool TRUST = false, bool GL = false>
__device__ inline bool csr_wave_uniform(const Csr& A, const double* __restrict__ x, int32_t s, int lane,
                                        double2* vs, int2* cs, int32_t ks, int32_t ke, int32_t r, const Epi& epi,
                                        const typename Epi::P& pe) {
    constexpr int P = LEN / 2;   // pairs per row == 16-byte loads per lane
    if constexpr (GL) {
        static_assert(TRUST, "LDS-DMA staging only for table-trusted waves");
        // values: P instructions of 64 x 16 B; columns: LEN / 4 whole instructions and, for LEN = 10, half of one
#pragma unroll
        for (int j = 0; j < P; ++j) glds16(A.va + s + 2 * (lane + 64 * j), vs + 64 * j);
#pragma unroll
        for (int j = 0; j < LEN / 4; ++j) glds16(A.ci + s + 4 * (lane + 64 * j), cs + 128 * j);
        if constexpr (LEN % 4 != 0) {
            if (lane < 32) glds16(A.ci + s + 4 * (lane + 64 * (LEN / 4)), cs + 128 * (LEN / 4));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        double2 v[P];
        int2 cc[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int32_t k = s + 2 * (lane + 64 * j);
            v[j] = ld_matrix<kCsrNT>(reinterpret_cast<const double2*>(A.va + k));
            cc[j] = ld_matrix<kCsrNT>(reinterpret_cast<const int2*>(A.ci + k));
        }
        // (a compiler memory barrier: the loads above may not sink below the check, which would serialise them
        // behind the row_ptr loads again; it emits no instruction and no wait)
        asm volatile("" ::: "memory");
        if (!TRUST && !__all(ke - ks == LEN)) return false;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            vs[lane + 64 * j] = v[j];
            cs[lane + 64 * j] = cc[j];
        }
    }
    wave_lds_sync();
    const int p0 = lane * P;
    int2 c[P];
#pragma unroll
    for (int i = 0; i < P; ++i) c[i] = cs[p0 + i];
    double x0[P], x1[P];
    if constexpr (XB) {
        const auto xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(x), (short)0, A.ncols * 8, 0x00020000);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            x0[i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, c[i].x * 8, 0, 0));
            x1[i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, c[i].y * 8, 0, 0));
        }
    } else {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            x0[i] = x[c[i].x];
            x1[i] = x[c[i].y];
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const double2 q = vs[p0 + i];
        acc += q.x * x0[i];
        acc += q.y * x1[i];
    }
    epi.template apply<kCsrNT>(r, acc, pe);   // every lane holds a row here
    return true;
}

// The wave table (mpbp_rowblocks.table; mpbp_set_csr_table(0) ignores it): a wave flagged uniform starts its matrix loads
// right after one scalar load of its block's 32-byte table entry -- no dependent row-range load, no row_ptr reads.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const i32x4 ci32x4;
template <class Epi>
__global__ void __launch_bounds__(kBlock) k_csr_wave(Csr A, const double* __restrict__ x,
                                                     const int2* __restrict__ blocks, int nblocks,
                                                     const int32_t* __restrict__ table, Epi epi) {
    __shared__ double2 vstage[kBlock / 64][kWaveCap / 2];
    __shared__ int2 cstage[kBlock / 64][kWaveCap / 2];
    const int b = xcd_swizzle(blockIdx.x, nblocks);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (table && A.ncols > 0 && A.ncols < (1 << 28)) {
        const i32x4 t0 = ((ci32x4*)table)[2 * b], t1 = ((ci32x4*)table)[2 * b + 1];
        const int32_t ra = t0.x + 64 * w;
        if (ra >= t0.y) return;
        const int len = (t1.w >> (8 * w)) & 255;
        if (len) {
            const int32_t s = w == 0 ? t0.z : w == 1 ? t0.w : w == 2 ? t1.x : t1.y;
            const int32_t r = ra + lane;
            const typename Epi::P pe = epi.pre(r);
            constexpr bool XB = true;
            if ((s & 3) == 0) {   // 16-byte aligned column chunk: LDS-DMA staging
                if (len == 12) csr_wave_uniform<12, XB, Epi, true, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
                else if (len == 10) csr_wave_uniform<10, XB, Epi, true, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
                else csr_wave_uniform<8, XB, Epi, true, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
                return;
            }
            if (len == 12) csr_wave_uniform<12, XB, Epi, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
            else if (len == 10) csr_wave_uniform<10, XB, Epi, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
            else csr_wave_uniform<8, XB, Epi, true>(A, x, s, lane, vstage[w], cstage[w], 0, 0, r, epi, pe);
            return;
        }
    }
    const int2 blk = blocks[b];
    const int32_t ra = __builtin_amdgcn_readfirstlane(blk.x + 64 * w);
    if (ra >= blk.y) return;   // waves are independent: no workgroup barrier below
    const int32_t rb = min(ra + 64, blk.y);
    const int32_t r = ra + lane;
    const bool live = r < rb;
    // the wave's entry range through scalar loads (their own counter: the matrix loads of the uniform path wait for
    // them alone), the rows' bounds through unconditional vector loads (lanes past the block re-read row ra)
    const int32_t s = ld_uniform_i32(A.rp, ra), e = ld_uniform_i32(A.rp, rb);
    const int32_t rr = live ? r : ra;
    const int32_t ks = A.rp[rr], ke0 = A.rp[rr + 1];
    const int32_t ke = live ? ke0 : ks;   // (an empty row for lanes past the block)
    typename Epi::P pe{};
    if (live) pe = epi.pre(r);
    double acc = 0.0;
    double2* vs = vstage[w];
    const double* vs1 = reinterpret_cast<const double*>(vs);
    {
        const int32_t len = (e - s) >> 6;   // wave-uniform
        if (rb - ra == 64 && ((e - s) & 63) == 0 && (s & 1) == 0 && (len == 8 || len == 10 || len == 12)) {
            constexpr bool XB = true;
            bool done;
            if (XB && A.ncols > 0 && A.ncols < (1 << 28))
                done = len == 12 ? csr_wave_uniform<12, XB>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe)
                                 : (len == 10 ? csr_wave_uniform<10, XB>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe)
                                              : csr_wave_uniform<8, XB>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe));
            else
                done = len == 12 ? csr_wave_uniform<12, false>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe)
                                 : (len == 10 ? csr_wave_uniform<10, false>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe)
                                              : csr_wave_uniform<8, false>(A, x, s, lane, vs, cstage[w], ks, ke, r, epi, pe));
            if (done) return;
        }
    }
    for (int32_t cb = s & ~1; cb < e; cb += kWaveCap) {
        double2 v[kWavePairs];
        int2 cc[kWavePairs];
#pragma unroll
        for (int j = 0; j < kWavePairs; ++j) {
            const int32_t k = cb + 2 * (lane + 64 * j);
            if (k + 1 < e) {
                v[j] = ld_matrix<kCsrNT>(reinterpret_cast<const double2*>(A.va + k));
                cc[j] = ld_matrix<kCsrNT>(reinterpret_cast<const int2*>(A.ci + k));
            } else if (k < e) {
                v[j] = make_double2(A.va[k], 0.0);
                cc[j] = make_int2(A.ci[k], 0);
            } else {
                v[j] = make_double2(0.0, 0.0);
                cc[j] = make_int2(0, 0);
            }
        }
        int32_t t = max(ks, cb) - cb;                       // this lane's row within the chunk
        const int32_t tend = min(ke, cb + kWaveCap) - cb;
        if (cb != (s & ~1)) wave_lds_sync();   // the previous chunk's reads are done
        int2* cs = cstage[w];
        const int32_t* cs1 = reinterpret_cast<const int32_t*>(cs);
#pragma unroll
        for (int j = 0; j < kWavePairs; ++j) {
            vs[lane + 64 * j] = v[j];
            cs[lane + 64 * j] = cc[j];
        }
        wave_lds_sync();
        if ((t & 1) && t < tend) {   // odd start: one entry, then whole pairs
            acc += vs1[t] * x[cs1[t]];
            ++t;
        }
        for (; t < tend; t += 2 * kRowBatch) {
            const int32_t p0 = t >> 1;
            int2 c[kRowBatch];
            double x0[kRowBatch], x1[kRowBatch];
#pragma unroll
            for (int i = 0; i < kRowBatch; ++i) c[i] = (t + 2 * i < tend) ? cs[p0 + i] : make_int2(0, 0);
#pragma unroll
            for (int i = 0; i < kRowBatch; ++i) {
                x0[i] = (t + 2 * i < tend) ? x[c[i].x] : 0.0;
                x1[i] = (t + 2 * i + 1 < tend) ? x[c[i].y] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < kRowBatch; ++i) {
                if (t + 2 * i < tend) {
                    const double2 q = vs[p0 + i];
                    acc += q.x * x0[i];
                    if (t + 2 * i + 1 < tend) acc += q.y * x1[i];
                }
            }
        }
    }
    if (live) epi.template apply<kCsrNT>(r, acc, pe);
}

// ---------------------------------------------------- HBM calibration (measurement only) ----
// The bench's same-run reference rates for the CSR SpMV roofline (mpbp_hbm_stream): mode 0 reads `bytes` once in order
// (16 B per lane, nontemporal, 16 KiB per workgroup); mode 1 the SpMV's own stream shape without its x gathers -- per
// 64-lane wave 9 KiB read in order and 64 doubles written (nontemporal), as a wave of 64 twelve-entry rows moves.
__global__ void __launch_bounds__(kBlock) k_hbm_read(const f64x2* __restrict__ p, int64_t n16, double* sink) {
    const int64_t base = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x) * 1024 + threadIdx.x;
    f64x2 acc = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + 256 * j;
        if (i < n16) acc += __builtin_nontemporal_load(p + i);
    }
    if (acc.x == 1234.5678 && acc.y == -8765.4321) sink[threadIdx.x] = acc.x;   // keeps the loads; never taken on data
}
__global__ void __launch_bounds__(kBlock) k_hbm_readwrite(const f64x2* __restrict__ p, int64_t nwaves, double* y) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x) * 4 + w;
    if (wv >= nwaves) return;
    const f64x2* q = p + wv * 576;
    f64x2 acc = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 9; ++j) acc += __builtin_nontemporal_load(q + lane + 64 * j);
    __builtin_nontemporal_store(acc.x + acc.y, y + wv * 64 + lane);
}

// ---------------------------------------------------- CSR, segmented reduction ----
// The same product under north_star's value bar instead of the oracle's order: identical row_ptr / col_idx
// handling, row sums within 1e-12 (relative infinity norm) of the sequential ones (np.matmul's BLAS sums are
// not sequential either, apply.py:72).  A uniform wave (64 rows of LEN = 2P entries from an even start, as in
// k_csr_wave) needs no LDS transposition: each row's P entry pairs sit in P consecutive lanes of a G-lane group
// (G = 4 for P = 4, else 8; lanes P..G-1 of a group repeat the group's last pair and add 0), a wave-instruction
// covers 64/G whole rows (contiguous 16-byte loads), every lane multiplies its own pair (x gathered by its own
// columns), and the group sums its pairs by DPP cross-lane adds (half-row mirror, then the two quad swaps; every
// lane of the group ends with the same bits, commutativity).  The row sums then go through 512 B of LDS so the
// epilogue runs one row per lane.  LDS 2 KiB per workgroup instead of 36 KiB: occupancy is set by registers.
// Non-uniform waves take a plain lane-per-row loop (correct, not fast: tree order is for stencil operators).
template <int CTRL>
__device__ inline double dpp_f64(double v) {
    const int2 h = __builtin_bit_cast(int2, v);
    const int lo = __builtin_amdgcn_update_dpp(0, h.x, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, h.y, CTRL, 0xf, 0xf, false);
    return __builtin_bit_cast(double, make_int2(lo, hi));
}
constexpr int kDppQuadSwap2 = 0x4e;      // quad_perm [2,3,0,1]
constexpr int kDppQuadSwap1 = 0xb1;      // quad_perm [1,0,3,2]
constexpr int kDppHalfMirror = 0x141;    // row_half_mirror: lane k <- lane 7-k within 8

template <int LEN, class Epi>
__device__ inline bool csr_seg_uniform(const Csr& A, const double* __restrict__ x, int32_t s, int lane,
                                       double* ys, int32_t ks, int32_t ke, int32_t r, const Epi& epi,
                                       const typename Epi::P& pe) {
    constexpr int P = LEN / 2;               // entry pairs per row
    constexpr int G = P <= 4 ? 4 : 8;        // lanes per row group
    constexpr int RPI = 64 / G;              // rows per wave-instruction
    constexpr int NI = 64 / RPI;             // wave-instructions for the wave's 64 rows
    const int k = lane % G, rg = lane / G;
    const int kc = k < P ? k : P - 1;        // idle lanes re-read the group's last pair (same cache line)
    double2 v[NI];
    int2 c[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int32_t q = s + 2 * ((j * RPI + rg) * P + kc);
        v[j] = ld_matrix<kCsrNT>(reinterpret_cast<const double2*>(A.va + q));
        c[j] = ld_matrix<kCsrNT>(reinterpret_cast<const int2*>(A.ci + q));
    }
    asm volatile("" ::: "memory");           // keep the matrix loads ahead of the row check (as csr_wave_uniform)
    if (!__all(ke - ks == LEN)) return false;
    const auto xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(x), (short)0, A.ncols * 8, 0x00020000);
    double t[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const double x0 = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, c[j].x * 8, 0, 0));
        const double x1 = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, c[j].y * 8, 0, 0));
        // (a bit mask, not a branch: the gathers of idle lanes stay unconditional, so they issue back to back)
        const uint64_t keep = k < P ? ~0ull : 0ull;
        t[j] = __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, __builtin_fma(v[j].y, x1, v[j].x * x0)) & keep);
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        if constexpr (G == 8) t[j] += dpp_f64<kDppHalfMirror>(t[j]);
        t[j] += dpp_f64<kDppQuadSwap2>(t[j]);
        t[j] += dpp_f64<kDppQuadSwap1>(t[j]);
        if (k == 0) ys[j * RPI + rg] = t[j];
    }
    wave_lds_sync();
    epi.template apply<kCsrNT>(r, ys[lane], pe);
    return true;
}

template <class Epi>
__global__ void __launch_bounds__(kBlock) k_csr_seg(Csr A, const double* __restrict__ x,
                                                    const int2* __restrict__ blocks, int nblocks, Epi epi) {
    __shared__ double ystage[kBlock / 64][64];
    const int b = xcd_swizzle(blockIdx.x, nblocks);
    const int2 blk = blocks[b];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t ra = __builtin_amdgcn_readfirstlane(blk.x + 64 * w);
    if (ra >= blk.y) return;
    const int32_t rb = min(ra + 64, blk.y);
    const int32_t r = ra + lane;
    const bool live = r < rb;
    const int32_t s = ld_uniform_i32(A.rp, ra), e = ld_uniform_i32(A.rp, rb);
    const int32_t rr = live ? r : ra;
    const int32_t ks = A.rp[rr], ke0 = A.rp[rr + 1];
    const int32_t ke = live ? ke0 : ks;
    typename Epi::P pe{};
    if (live) pe = epi.pre(r);
    const int32_t len = (e - s) >> 6;
    if (rb - ra == 64 && ((e - s) & 63) == 0 && (s & 1) == 0 && A.ncols > 0 && A.ncols < (1 << 28)) {
        // every lane is live here: the raw row end ke0, so no select on it waits for the row_ptr loads before
        // the matrix loads issue
        bool done = false;
        if (len == 12) done = csr_seg_uniform<12>(A, x, s, lane, ystage[w], ks, ke0, r, epi, pe);
        else if (len == 10) done = csr_seg_uniform<10>(A, x, s, lane, ystage[w], ks, ke0, r, epi, pe);
        else if (len == 8) done = csr_seg_uniform<8>(A, x, s, lane, ystage[w], ks, ke0, r, epi, pe);
        if (done) return;
    }
    double acc = 0.0;
    for (int32_t kk = ks; kk < ke; ++kk) acc += A.va[kk] * x[A.ci[kk]];
    if (live) epi.template apply<kCsrNT>(r, acc, pe);
}

// ---------------------------------------------- CSR, G lanes per row (small levels) ----
// The multigrid's small levels (<= 64^2 cells per field: 1-16 K rows of 20-46 entries) are latency-bound, not
// bandwidth-bound: one lane per row walks its row in batches, each batch a matrix load -> x gather chain, so a
// 4 K-row sweep took ~9 us for 2 MB.  Here G lanes share a row: each loads J of its entries (entries k, k + G, ...;
// all loads of the row in flight at once), gathers x and forms the products v * x in parallel, writes them to
// LDS, and the group's first lane adds them left to right from 0.0 -- the CSR row's sequential sum, bit for bit
// (same products, same order, no FMA).  One latency chain per row instead of one per batch, and G times the lanes
// for the few rows.  Rows longer than G * J entries take several chunks (correct for any CSR).  A DZ epilogue
// reads the Chebyshev direction as +0.0 without loading it (the smoother's restart after a coarse correction,
// same IEEE operations as a zeroed vector: no memset launch).
constexpr int kGrpJ = 8;   // entries per lane per chunk
template <class Epi>
struct EpiZeroD : Epi {   // Epi = EpiCheb: d read as +0.0 (never loaded)
    using P = typename Epi::P;
    __device__ P pre(int32_t r) const {
        return {this->xin[r], ld_stream(this->b + r), this->diag ? this->diag[r] : 0.0, 0.0,
                this->sub ? ld_stream(this->sub + r) : 0.0};
    }
    // the stencil kernels' form (x and the diagonal from the stencil itself)
    __device__ P pre_lite(int32_t r) const {
        return {0.0, Epi::kBX ? 0.0 : ld_stream(this->b + r), 0.0, 0.0,
                (this->has_sub() && !Epi::kSubLate) ? ld_stream(this->sub + r) : 0.0};
    }
};
// The first Chebyshev sweep from x = 0 with the init pass folded in (XS = XInit gathers x0 = c2_0 (b / diag) at every
// column, the same expression k_cheb_init stores): the epilogue's x and direction are the row's own x0.
struct EpiChebFirstGrp : EpiChebFirst {
    const double* diag;
    double c2_0;
    __device__ P pre(int32_t r) const {
        P p = EpiChebFirst::pre(r);
        p.dg = diag[r];
        p.x = c2_0 * (p.b / p.dg);
        return p;
    }
};
template <int G, class XS, class Epi>
__global__ void __launch_bounds__(kBlock) k_csr_grp(Csr A, int32_t nrows, XS xs, Epi epi) {
    constexpr int RPB = kBlock / G, CAP = G * kGrpJ;
    __shared__ double prod[RPB * CAP];
    const int g = threadIdx.x / G, k = threadIdx.x % G;
    const int32_t r = xcd_swizzle(blockIdx.x, gridDim.x) * RPB + g;
    const bool live = r < nrows;
    const int32_t rr = live ? r : nrows - 1;
    const int32_t ks = A.rp[rr], ke = live ? A.rp[rr + 1] : ks;
    typename Epi::P pe{};
    if (live && k == 0) pe = epi.pre(r);
    double* pr = prod + g * CAP;
    double acc = 0.0;
    for (int32_t cb = ks; cb < ke; cb += CAP) {
        double v[kGrpJ];
        int32_t c[kGrpJ];
#pragma unroll
        for (int j = 0; j < kGrpJ; ++j) {
            const int32_t e = cb + k + G * j;
            const bool in = e < ke;
            v[j] = in ? A.va[e] : 0.0;
            c[j] = in ? A.ci[e] : 0;
        }
        double p[kGrpJ];
#pragma unroll
        for (int j = 0; j < kGrpJ; ++j) p[j] = v[j] * xs(c[j]);
        if (cb != ks) wave_lds_sync();   // the previous chunk's sums have read their slots
#pragma unroll
        for (int j = 0; j < kGrpJ; ++j) pr[k + G * j] = p[j];
        wave_lds_sync();                 // a group never spans two waves (G divides 64)
        if (k == 0) {
            const int32_t cnt = min(ke - cb, (int32_t)CAP);
            for (int32_t i = 0; i < cnt; ++i) acc += pr[i];
        }
    }
    if (live && k == 0) epi(r, acc, pe);
}

// ------------------------------------------------------------ stencil-values layout ----
// The multigrid's large Galerkin levels (F level 1 at 1024^2: 1 M rows x 40 entries) stream 12 B per entry on SELL;
// their rows all hold the same (field, dr, dc) offsets (translation-invariant operator on a periodic grid), so the
// column indices are rebuilt as row + delta[f][s] and only the values are streamed, slot-major (coalesced per slot
// across consecutive rows, nontemporal).  One thread per interior row (threads enumerate the interior cells of
// every field densely, so no wave mixes the two paths): K products in slot order = the CSR row's column order;
// the x gathers need no column load, so they issue beside the value loads.  Then one thread per edge row (within
// `reach` of the periodic edge, where the wrapped columns sort differently): the CSR row, left to right.  Both the
// CSR SpMV's additions exactly (bit-identical), at 8 B instead of 12 B per entry for all but the edge rows.
struct Svl {
    int nf, m, R, K;
    const int32_t* delta;
    const double* vals;
    const int32_t* edge;
    int n_edge;
};
constexpr int kSvB = 8;  // slots per batch (values + gathers in flight together)

constexpr int kSvMaxDelta = 256;     // nf * K
constexpr int kSvEdgeG = 8;          // lanes per edge row (k_csr_grp's scheme: one latency chain per row)
template <class XS, class Epi>
__global__ void __launch_bounds__(kBlock) k_svl(Svl V, Csr A, int32_t nrows, XS xs, Epi epi) {
    __shared__ int32_t sdelta[kSvMaxDelta];
    __shared__ double prod[kBlock * kGrpJ];
    for (int i = threadIdx.x; i < V.nf * V.K; i += kBlock) sdelta[i] = V.delta[i];
    __syncthreads();
    // interior: one thread per pair of horizontally adjacent cells (reach is even, so W = m - 2 reach is even and a
    // pair starts on an even row id): 16-byte value loads, two rows' products, two ordered sums
    const int W = V.m - 2 * V.R;
    const int W2 = W >> 1;
    const int32_t per = W2 * W;                        // pairs per field
    const int32_t ni = V.nf * per;
    // the edge rows' latency-bound CSR chains in the first-dispatched workgroups (round-robin over the XCDs), the
    // interior pairs behind them (XCD-contiguous runs): otherwise the edge chains start last, behind the stream
    // (multigrid apply 1.767 -> 1.731 ms, A/B on one box)
    const int32_t nb_edge = (V.n_edge * kSvEdgeG + kBlock - 1) / kBlock;
    const bool eb = (int32_t)blockIdx.x < nb_edge;
    const int32_t t0 = (int32_t)blockIdx.x * kBlock + (int32_t)threadIdx.x;
    const int32_t t = eb ? ni : (int32_t)xcd_swizzle(blockIdx.x - nb_edge, gridDim.x - nb_edge) * kBlock + (int32_t)threadIdx.x;
    const bool edge_ok = eb && t0 < V.n_edge * kSvEdgeG;
    if (t < ni) {
        const uint32_t f = (uint32_t)t / (uint32_t)per;
        const uint32_t i = (uint32_t)t - f * (uint32_t)per;
        const uint32_t q = i / (uint32_t)W2;
        const int r = V.R + (int)q, c = V.R + 2 * (int)(i - q * (uint32_t)W2);
        const int32_t row = ((int32_t)f * V.m + r) * V.m + c;
        const typename Epi::P pe0 = epi.pre(row), pe1 = epi.pre(row + 1);
        const int32_t* dl = sdelta + f * V.K;
        const double* vp = V.vals + row;
        double a0 = 0.0, a1 = 0.0;
        for (int s0 = 0; s0 < V.K; s0 += kSvB) {
            f64x2 v[kSvB];
            double x0[kSvB], x1[kSvB];
#pragma unroll
            for (int j = 0; j < kSvB; ++j) {
                const int sj = min(s0 + j, V.K - 1);   // (a tail batch re-reads the last slot and discards it)
                v[j] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(vp + (int64_t)sj * nrows));
                const int32_t col = row + dl[sj];
                x0[j] = xs(col);
                x1[j] = xs(col + 1);
            }
#pragma unroll
            for (int j = 0; j < kSvB; ++j)
                if (s0 + j < V.K) {
                    a0 += v[j].x * x0[j];
                    a1 += v[j].y * x1[j];
                }
        }
        epi(row, a0, pe0);
        epi(row + 1, a1, pe1);
    } else if (edge_ok) {
        const int64_t u = t0;
        // edge row: kSvEdgeG lanes load its CSR entries at once and form the products, the first lane sums them in
        // order (k_csr_grp)
        constexpr int G = kSvEdgeG, CAP = G * kGrpJ;
        const int32_t row = V.edge[u / G];
        const int k = (int)(u % G);
        double* pr = prod + (threadIdx.x / G) * CAP;
        typename Epi::P pe{};
        if (k == 0) pe = epi.pre(row);
        const int32_t ks = A.rp[row], ke = A.rp[row + 1];
        double acc = 0.0;
        for (int32_t cb = ks; cb < ke; cb += CAP) {
            double p[kGrpJ];
#pragma unroll
            for (int j = 0; j < kGrpJ; ++j) {
                const int32_t e = cb + k + G * j;
                const bool in = e < ke;
                p[j] = (in ? A.va[e] : 0.0) * xs(in ? A.ci[e] : row);
            }
            if (cb != ks) wave_lds_sync();
#pragma unroll
            for (int j = 0; j < kGrpJ; ++j) pr[k + G * j] = p[j];
            wave_lds_sync();
            if (k == 0) {
                const int32_t cnt = min(ke - cb, (int32_t)CAP);
                for (int32_t i = 0; i < cnt; ++i) acc += pr[i];
            }
        }
        if (k == 0) epi(row, acc, pe);
    }
}

// ------------------------------------------------------------------ SELL-64 ----
// Sliced ELLPACK with one wavefront per slice: a slice is <= 64 consecutive rows, its entries
// stored column-major in pairs -- pair-row j of the slice holds entries (2j, 2j+1) of every row,
// one double2 / int2 per lane -- so each wave-instruction reads 1 KiB of values and 512 B of
// column indices contiguously, and each lane owns one row: no LDS, no barrier, no reduction
// across lanes.  Entries keep their CSR order, so row sums stay bit-exact with the oracle.
// slices[s] = {row0, rows, width, first pair-row}; row_len[r] = CSR length of row r (< 256).
struct Sell {
    const int4* slices;
    const uint8_t* rlen;
    const double2* val;
    const int2* col;
};

constexpr int kSellPairs = 8;   // rows of up to 16 entries take the fully unrolled path

template <class Epi>
__global__ void __launch_bounds__(kBlock) k_sell_rows(Sell S, const double* __restrict__ x, int nslices,
                                                      Epi epi) {
    const int b = xcd_swizzle(blockIdx.x, gridDim.x);
    const int sidx = b * (kBlock / 64) + (int)(threadIdx.x >> 6);
    if (sidx >= nslices) return;
    const int lane = threadIdx.x & 63;
    const int4 sl = S.slices[sidx];
    const int32_t r = sl.x + lane;
    const bool live = lane < sl.y;
    const int len = live ? (int)S.rlen[r] : 0;
    typename Epi::P pe{};
    if (live) pe = epi.pre(r);
    const int np = (sl.z + 1) >> 1;
    const double2* vp = S.val + (size_t)sl.w * 64 + lane;
    const int2* cp = S.col + (size_t)sl.w * 64 + lane;
    double acc = 0.0;
    // pair-rows [j0, j0 + kSellPairs): every load of the batch first (slice padding is zero, so loads past a
    // row's end are harmless), then the x gathers, then the products added in CSR order.  Rows of up to 16
    // entries take one batch; longer ones (multigrid coarse operators: 20-50 entries) loop over batches.
    auto batch = [&](int j0) {
        double2 v[kSellPairs];
        int2 c[kSellPairs];
#pragma unroll
        for (int j = 0; j < kSellPairs; ++j) {
            if (j0 + j < np) {   // wave-uniform
                v[j] = ld_matrix<kSellNT>(vp + (size_t)(j0 + j) * 64);
                c[j] = ld_matrix<kSellNT>(cp + (size_t)(j0 + j) * 64);
            } else {
                v[j] = make_double2(0.0, 0.0);
                c[j] = make_int2(0, 0);
            }
        }
        double x0[kSellPairs], x1[kSellPairs];
#pragma unroll
        for (int j = 0; j < kSellPairs; ++j) {
            x0[j] = (2 * (j0 + j) < len) ? x[c[j].x] : 0.0;
            x1[j] = (2 * (j0 + j) + 1 < len) ? x[c[j].y] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < kSellPairs; ++j) {
            if (2 * (j0 + j) < len) acc += v[j].x * x0[j];
            if (2 * (j0 + j) + 1 < len) acc += v[j].y * x1[j];
        }
    };
    if (np <= kSellPairs) {
        batch(0);
    } else {
        for (int j0 = 0; j0 < np; j0 += kSellPairs) batch(j0);
    }
    if (live) epi.template apply<kSellNT>(r, acc, pe);
}

// ------------------------------------------------------------- F stencil ----
// Matrix-free rows of F = XI + d_u blockdiag(eta_n L_n, eta_s L_s): the ten entries of a row are
// recomputed from the thn tables (L1/L2-resident) with exactly the assembly's arithmetic
// (phase_L_row / F_row above) and their products summed in the assembled row's column order -- the same
// IEEE operations as a sweep over the assembled F, without streaming its 12 bytes x 10 entries per row
// from HBM.  Needs n >= 3 (no coinciding periodic neighbours).
//
// Column order on the periodic edge.  A stencil's products are listed in the interior's sorted-column order;
// on the grid's edge a wrapped neighbour moves (row -1 -> n-1 sorts last, row n -> 0 first, and likewise for
// columns).  Instead of sorting, the edge form adds every product at each position it can occupy, with the
// positions it does not occupy on this lane contributing -0.0 -- the exact identity of IEEE addition in
// round-to-nearest (x + -0.0 == x for every x, signed zeros included) -- so the sum performs exactly the
// sorted row's additions, with no sorting network and the same code on every lane.
struct Wrap {
    bool r0, rl, c0, cl;   // the cell's grid row is 0 / n-1, its column 0 / n-1
};
__device__ inline double opt(bool c, double p) { return c ? p : -0.0; }
// Five-point products p = {N, W, C, E, S} (interior column order), added to acc in the row's column order.
template <bool EDGE>
__device__ inline double add5(double acc, const double* p, const Wrap& w) {
    if constexpr (!EDGE) {
#pragma unroll
        for (int t = 0; t < 5; ++t) acc += p[t];
        return acc;
    }
    acc += opt(w.rl, p[4]);    // S wrapped to row 0: first
    acc += opt(!w.r0, p[0]);   // N
    acc += opt(w.cl, p[3]);    // E wrapped to column 0: before W
    acc += opt(!w.c0, p[1]);   // W
    acc += p[2];               // C
    acc += opt(!w.cl, p[3]);   // E
    acc += opt(w.c0, p[1]);    // W wrapped to column n-1: after E
    acc += opt(!w.rl, p[4]);   // S
    acc += opt(w.r0, p[0]);    // N wrapped to row n-1: last
    return acc;
}
// 2 x 2 block products p = {a_lo, a_hi, b_lo, b_hi} (rows a above b, columns lo left of hi): the lower row
// comes first when it wraps (bwrap), the high column first when the pair wraps (cwrap).
template <bool EDGE>
__device__ inline double add4(double acc, const double* p, bool bwrap, bool cwrap) {
    if constexpr (!EDGE) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc += p[t];
        return acc;
    }
    acc += opt(bwrap && cwrap, p[3]);
    acc += opt(bwrap, p[2]);
    acc += opt(bwrap && !cwrap, p[3]);
    acc += opt(cwrap, p[1]);
    acc += p[0];
    acc += opt(!cwrap, p[1]);
    acc += opt(!bwrap && cwrap, p[3]);
    acc += opt(!bwrap, p[2]);
    acc += opt(!bwrap && !cwrap, p[3]);
    return acc;
}

// Offset of local grid row lr (-h <= lr < L + h) of field f in an nf-field vector of the row-partition
// layout: the owned rows field-major, then h ghost rows above of every field (increasing row order), then
// h ghost rows below of every field.
__device__ inline int32_t ext_row(int nf, int f, int lr, int L, int h, int n) {
    if (lr >= 0 && lr < L) return (f * L + lr) * n;
    return nf * L * n + (lr < 0 ? f * h + h + lr : nf * h + f * h + lr - L) * n;
}

struct FStencilDev {
    static constexpr bool kFast = false;   // FStencilFast: tolerance-mode rows (rows4 / rdiag4, reciprocal diagonals)
    int n;
    double xi, eta_n, eta_s, c, d_u;
    const double* cell;
    const double* uface;
    const double* vface;
    // grid constants, evaluated once on the host exactly as the assembly evaluates them on the device
    double dxdx;   // dx * dx
    double idx2;   // 1.0 / (dx * dx)   (== 1.0 / (dy * dy), 1.0 / (dx * dy): dx == dy)
    double midy2;  // -1.0 / (dy * dy)
    // row partition: this rank owns grid rows [r0, r0 + L) of each of the 4 velocity fields; the ghosts
    // follow the 4*L*n owned entries: h rows above of every field, then h rows below of every field.
    // One GPU: r0 = 0, L = n, h = 0.
    int r0, L, h, which;
    int pow2;      // n is a power of two: dx * dx is a power of two and v / (dx * dx) == v * idx2 exactly
    int ext = 0;   // which = 3: ghost rows computed on each side
    int oh = 0;    // ghost depth of the output's layout (== h)
    double ce0 = 0.0, ce1 = 0.0;   // pow2: eta_n * idx2, eta_s * idx2 (exact: idx2 is a power of two)

    __device__ int wrap(int a) const { return a < 0 ? a + n : (a >= n ? a - n : a); }
    // index in x of (field f, grid row gr, column 0) for gr in [r0 - h, r0 + L + h)
    __device__ int32_t xrow(int f, int gr) const {
        if (h == 0) return (f * n + wrap(gr)) * n;
        return ext_row(4, f, gr - r0, L, h, n);
    }
    // k_march policy: the 4 velocity fields staged, the cell's 4 rows out; per cell, the u- and v-face
    // thn values are requested with the epilogue operands (before the barrier), not inside the rows
    static constexpr int NF = 4, NOUT = 4;
    struct Cell { double face[2]; };
    __device__ Cell cell_pre(int gr, int gc) const { return {{uface[gr * n + gc], vface[gr * n + gc]}}; }
    __device__ int32_t out_row(int f, int lr, int gc) const {
        return (lr >= 0 && lr < L ? (f * L + lr) * n : ext_row(4, f, lr, L, oh, n)) + gc;
    }
    template <bool EDGE, class TA, class XA>
    __device__ double row(int f, int gr, int gc, const TA& ta, const XA& xa, double* fd, const Cell& cl) const;
    // k_march_init: the face thn a staged point's diagonal needs, and that diagonal
    struct Stage { double face[2]; };
    __device__ Stage stage_pre(int gr, int gcw) const {
        const int32_t k = wrap(gr) * n + gcw;
        return {{uface[k], vface[k]}};
    }
    template <class TA>
    __device__ double stage_diag(int f, int gr, int gc, const TA& ta, const Stage& s) const;
};

// The diagonal of an F row (phase_L_row's diagonal + XI + the c-weighted identity, F_row), with the
// intermediate thn averages the row's off-diagonal entries reuse.  One definition serves the row itself
// (f_row) and the first inner sweep's staged x0 = c2 b / diag (k_march_init), so both see the same bits.
// M: f_row's compile-time parameter identities.
template <int M>
struct FDiagCommon {
    __device__ static double dmul(const FStencilDev& P, double y) { return (M & 1) ? -y : P.d_u * y; }
    __device__ static double emul(const FStencilDev& P, int p, double y) {
        const bool eta1 = p ? (M & 4) != 0 : (M & 2) != 0;
        return eta1 ? y : (p ? P.eta_s : P.eta_n) * y;
    }
};
template <int M>
struct FDiagU : FDiagCommon<M> {   // u row at (gr, gc): preconditioner.py:100-179
    double iph_jph, iph_jmh, xi_ii, fd;
    template <class TA>
    __device__ FDiagU(const FStencilDev& P, int p, const TA& ta, int gr, int gc, double th) {
        const double tij = ta.T(p, gr, gc - 1), tip1j = ta.T(p, gr, gc);
        const double tijp1 = ta.T(p, gr - 1, gc - 1), tip1jp1 = ta.T(p, gr - 1, gc);
        const double tijm1 = ta.T(p, gr + 1, gc - 1), tip1jm1 = ta.T(p, gr + 1, gc);
        iph_jph = 0.25 * (tij + tijp1 + tip1jp1 + tip1j);
        iph_jmh = 0.25 * (tij + tip1j + tijm1 + tip1jm1);
        const double iph_j = 0.5 * (tij + tip1j);
        xi_ii = xi_of(P.xi, iph_j);
        const double wt = p ? P.c * (1.0 - th) : P.c * th;
        const double Ldiag = P.idx2 * (-tip1j - tij) + P.idx2 * (-iph_jph - iph_jmh);
        fd = (wt - this->dmul(P, xi_ii)) + this->dmul(P, this->emul(P, p, Ldiag));
    }
};
template <int M>
struct FDiagV : FDiagCommon<M> {   // v row at (gr, gc): preconditioner.py:182-295
    double tij, tijp1, imh_jph, iph_jph, xi_ii, fd;
    template <class TA>
    __device__ FDiagV(const FStencilDev& P, int p, const TA& ta, int gr, int gc, double th) {
        tij = ta.T(p, gr, gc);
        const double tip1j = ta.T(p, gr, gc + 1);
        tijp1 = ta.T(p, gr - 1, gc);
        const double tip1jp1 = ta.T(p, gr - 1, gc + 1);
        const double tim1j = ta.T(p, gr, gc - 1), tim1jp1 = ta.T(p, gr - 1, gc - 1);
        const double ip1_jph = 0.5 * (tij + tijp1);
        xi_ii = xi_of(P.xi, ip1_jph);
        const double wt = p ? P.c * (1.0 - th) : P.c * th;
        imh_jph = 0.25 * (tim1j + tim1jp1 + tij + tijp1);
        iph_jph = 0.25 * (tij + tip1j + tijp1 + tip1jp1);
        const double Ldiag = P.midy2 * (tijp1 + tij) - P.idx2 * (iph_jph + imh_jph);
        fd = (wt - this->dmul(P, xi_ii)) + this->dmul(P, this->emul(P, p, Ldiag));
    }
};

template <int M, class TA>
__device__ inline double f_stage_diag(const FStencilDev& P, int f, int gr, int gc, const TA& ta,
                                      const FStencilDev::Stage& s) {
    const int p = f >> 1;
    return (f & 1) == 0 ? FDiagU<M>(P, p, ta, gr, gc, s.face[0]).fd : FDiagV<M>(P, p, ta, gr, gc, s.face[1]).fd;
}
template <class TA>
__device__ inline double FStencilDev::stage_diag(int f, int gr, int gc, const TA& ta, const Stage& s) const {
    return f_stage_diag<0>(*this, f, gr, gc, ta, s);
}

// The ten entries of one F row, built in the assembled row's column order for interior points and
// sorted (with fixed networks) where periodic wrap-around reorders them.  TA::T(s, gr, gc) is thn of
// phase s at a cell, XA::X(f, gr, gc) the x entry of field f at a grid point (gr in [-1, n], gc in
// [-1, n]; the accessors wrap).  Same operations as phase_L_row / F_row, same summation order.
// M (exact parameter identities, compile time): bit 0 d_u == -1 (d_u * y is an exact negation, folded into
// the products as a sign), bit 1 eta_n == 1, bit 2 eta_s == 1 (eta * y == y exactly), bit 3 idx2 a power of
// two: eta * (idx2 * y) == y * (eta * idx2) for every y (idx2 * y and eta * idx2 are exact scalings, so both
// sides are the one rounding of the same real), one multiply per off-diagonal entry instead of two.  Every
// entry keeps the assembly's rounding; only multiplications whose result is exactly known are skipped.
template <bool EDGE, class TA, class XA, bool VIRT = false, int M = 0>
__device__ inline double f_row(const FStencilDev& P, int f, int gr, int gc, const TA& ta, const XA& xa,
                               double* fdiag, const double* face = nullptr) {
    const int n = P.n;
    const int p = f >> 1;
    const double idx2 = P.idx2;
    const double eta = p ? P.eta_s : P.eta_n;
    const bool eta1 = p ? (M & 4) != 0 : (M & 2) != 0;
    auto dmul = [&](double y) -> double { return (M & 1) ? -y : P.d_u * y; };   // d_u * y
    auto emul = [&](double y) -> double { return eta1 ? y : eta * y; };          // eta * y
    auto sc = [&](double y) -> double {                                          // eta * (idx2 * y)
        if constexpr ((M & 8) != 0) return eta1 ? idx2 * y : y * (p ? P.ce1 : P.ce0);
        else return emul(idx2 * y);
    };
    const int fu = 2 * p, fv = 2 * p + 1;
    const int32_t kc = VIRT ? P.wrap(gr) * n + P.wrap(gc) : gr * n + gc;   // VIRT: (gr, gc) may lie one cell outside
    auto T = [&](int r, int c) -> double { return ta.T(p, r, c); };
    const Wrap w{gr == 0, gr == n - 1, gc == 0, gc == n - 1};   // read by the EDGE form only
    double acc = 0.0;
    const double xcross = xa.X(f ^ 2, gr, gc);
    if ((f & 1) == 0) {   // u row: preconditioner.py:100-179
        const double tij = T(gr, gc - 1), tip1j = T(gr, gc);
        const double th = face ? face[0] : P.uface[kc];   // face: thn at the u / v face, loaded ahead
        const FDiagU<M> dd(P, p, ta, gr, gc, th);
        const double iph_jph = dd.iph_jph, iph_jmh = dd.iph_jmh, xi_ii = dd.xi_ii;
        const double fd = dd.fd;
        *fdiag = fd;
        // same field: N, W, C, E, S; the other component (v of this phase): (gr, gc-1), (gr, gc), (gr+1, gc-1),
        // (gr+1, gc)
        const double lo[5] = {dmul(sc(iph_jph)) * xa.X(fu, gr - 1, gc),
                              dmul(sc(tij)) * xa.X(fu, gr, gc - 1),
                              fd * xa.X(fu, gr, gc),
                              dmul((M & 8) ? sc(tip1j) : emul(P.pow2 ? tip1j * idx2 : tip1j / P.dxdx)) * xa.X(fu, gr, gc + 1),
                              dmul(sc(iph_jmh)) * xa.X(fu, gr + 1, gc)};
        const double hi[4] = {dmul(sc(tij - iph_jph)) * xa.X(fv, gr, gc - 1),
                              dmul(sc(-tip1j + iph_jph)) * xa.X(fv, gr, gc),
                              dmul(sc(iph_jmh - tij)) * xa.X(fv, gr + 1, gc - 1),
                              dmul(sc(tip1j - iph_jmh)) * xa.X(fv, gr + 1, gc)};
        const double vcross = dmul(xi_ii);
        if (p == 1) acc += vcross * xcross;
        acc = add5<EDGE>(acc, lo, w);
        acc = add4<EDGE>(acc, hi, w.rl, w.c0);
        if (p == 0) acc += vcross * xcross;
    } else {              // v row: preconditioner.py:182-295
        const double th = face ? face[1] : P.vface[kc];
        const FDiagV<M> dd(P, p, ta, gr, gc, th);
        const double tij = dd.tij, tijp1 = dd.tijp1;
        const double imh_jph = dd.imh_jph, iph_jph = dd.iph_jph, xi_ii = dd.xi_ii;
        const double fd = dd.fd;
        *fdiag = fd;
        // the other component (u of this phase): (gr-1, gc), (gr-1, gc+1), (gr, gc), (gr, gc+1); same field: N, W,
        // C, E, S
        const double lo[4] = {dmul(sc(tijp1 - imh_jph)) * xa.X(fu, gr - 1, gc),
                              dmul(sc(iph_jph - tijp1)) * xa.X(fu, gr - 1, gc + 1),
                              dmul(sc(imh_jph - tij)) * xa.X(fu, gr, gc),
                              dmul(sc(tij - iph_jph)) * xa.X(fu, gr, gc + 1)};
        const double hi[5] = {dmul(sc(tijp1)) * xa.X(fv, gr - 1, gc),
                              dmul(sc(imh_jph)) * xa.X(fv, gr, gc - 1),
                              fd * xa.X(fv, gr, gc),
                              dmul(sc(iph_jph)) * xa.X(fv, gr, gc + 1),
                              dmul(sc(tij)) * xa.X(fv, gr + 1, gc)};
        const double vcross = dmul(xi_ii);
        if (p == 1) acc += vcross * xcross;
        acc = add4<EDGE>(acc, lo, w.r0, w.cl);
        acc = add5<EDGE>(acc, hi, w);
        if (p == 0) acc += vcross * xcross;
    }
    return acc;
}

// ---- tolerance-mode F (plan numerics "fast"): north_star's 1e-12 bar instead of the assembly's bits ----
// The same operator with its four rows per cell regrouped around the phase-n thn at the cell centres and at the grid
// nodes (corner K(r, c): the average of the four cells around the node between rows r-1, r and columns c-1, c;
// phase s uses 1 - t), FMA-contracted.  With a = d_u eta idx2 and -d_u xi h (1 - h) the XI coupling (h: the face
// average), a u row (left / right cells A1 = T(r, c-1), A2 = T(r, c), nodes KN = K(r, c), KS = K(r+1, c)) is
//   F u = wt u_C - d_u xi_h (u_C - u_o) + a [KN (u_N - u_C + v2 - v1) + A1 (u_W - u_C + v1 - v3)
//                                           + A2 (u_E - u_C + v4 - v2) + KS (u_S - u_C + v3 - v4)]
// (v1..v4 = v(r, c-1), v(r, c), v(r+1, c-1), v(r+1, c)), diag = wt - d_u xi_h - a (A1 + A2 + KN + KS) -- the
// entries of preconditioner.py:100-179 collected per coefficient; a v row (:182-295) likewise with B1 = T(r-1, c),
// B2 = T(r, c), KW = K(r, c), KE = K(r, c+1) and u1..u4 = u(r-1, c), u(r-1, c+1), u(r, c), u(r, c+1).  Per row
// about 40 fp64 VALU operations (corners once per cell, a reciprocal diagonal by v_rcp_f64 and two Newton steps)
// instead of ~170 for the bit-exact rows; every value stays within a few ulp of the assembled row (numpy check:
// 3e-16 of max |F x|).  No periodic sorting: the sum has no order to reproduce.
__device__ inline double rcp_nr(double y) {
    double r = __builtin_amdgcn_rcp(y);
    double e = __builtin_fma(-y, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-y, r, 1.0);
    return __builtin_fma(r, e, r);
}
struct FStencilFast : FStencilDev {
    static constexpr bool kFast = true;
    struct Nb { double nw, nn, ne, w, c, e, sw, s; };   // phase-n thn around (r, c) (the 3 x 3 block minus (r+1, c+1))
    template <class TA>
    __device__ static Nb nb(const TA& ta, int gr, int gc) {
        return {ta.T(0, gr - 1, gc - 1), ta.T(0, gr - 1, gc), ta.T(0, gr - 1, gc + 1), ta.T(0, gr, gc - 1),
                ta.T(0, gr, gc), ta.T(0, gr, gc + 1), ta.T(0, gr + 1, gc - 1), ta.T(0, gr + 1, gc)};
    }
    // per-cell coefficients, phase n: A1 = w, A2 = B2 = c, B1 = nn; nodes kc = K(r, c), ks = K(r+1, c), ke = K(r, c+1)
    struct Co { double w, c, nn, kc, ks, ke, xu, xv; };
    __device__ Co coeffs(const Nb& t) const {
        const double wc = t.w + t.c;
        return coeffs_k(t.w, t.c, t.nn, wc, 0.25 * ((t.nw + t.nn) + wc), 0.25 * (wc + (t.sw + t.s)),
                        0.25 * ((t.nn + t.ne) + (t.c + t.e)));
    }
    // the same from the node averages (k_fsolve_w reads them from its LDS table); wc = w + c
    __device__ Co coeffs_k(double w, double c, double nn, double wc, double kc, double ks, double ke) const {
        Co k;
        k.w = w; k.c = c; k.nn = nn;
        k.kc = kc; k.ks = ks; k.ke = ke;
        const double hu = 0.5 * wc, hv = 0.5 * (nn + c);
        const double mx = -d_u * xi;             // -d_u xi h (1 - h): the same for both phases (h_s = 1 - h_n)
        k.xu = mx * (hu * (1.0 - hu));
        k.xv = mx * (hv * (1.0 - hv));
        return k;
    }
    __device__ double aco(int p) const { return d_u * (p ? eta_s : eta_n) * idx2; }
    // a cell's level-invariant row terms beside Co: the identity weights c thn_p at its u / v face, per phase
    struct W4 { double wu[2], wv[2]; };
    __device__ W4 weights(const Cell& cl) const {
        return {{c * cl.face[0], c * (1.0 - cl.face[0])}, {c * cl.face[1], c * (1.0 - cl.face[1])}};
    }
    // the four rows (u_n, v_n, u_s, v_s) of cell (gr, gc) from its coefficients k and weights w.  The XI coupling
    // xu (u_C - u_o) of the s phase is the n phase's negated (u_s - u_n = -(u_n - u_s) and xu (-y) = -(xu y) exactly in
    // round-to-nearest): one difference and one product serve both phases.
    template <class XA>
    __device__ void rows4_co(int gr, int gc, const Co& k, const W4& w, const XA& xa, double* acc) const {
        const double xdu = k.xu * (xa.X(0, gr, gc) - xa.X(2, gr, gc));
        const double xdv = k.xv * (xa.X(1, gr, gc) - xa.X(3, gr, gc));
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int fu = 2 * p, fv = 2 * p + 1;
            auto ph = [&](double t) { return p ? 1.0 - t : t; };
            const double a = aco(p);
            const double A1 = ph(k.w), A2 = ph(k.c), B1 = ph(k.nn), KC = ph(k.kc), KS = ph(k.ks), KE = ph(k.ke);
            const double uC = xa.X(fu, gr, gc), uN = xa.X(fu, gr - 1, gc), uS = xa.X(fu, gr + 1, gc);
            const double uW = xa.X(fu, gr, gc - 1), uE = xa.X(fu, gr, gc + 1), uNE = xa.X(fu, gr - 1, gc + 1);
            const double vC = xa.X(fv, gr, gc), vN = xa.X(fv, gr - 1, gc), vS = xa.X(fv, gr + 1, gc);
            const double vW = xa.X(fv, gr, gc - 1), vE = xa.X(fv, gr, gc + 1), vSW = xa.X(fv, gr + 1, gc - 1);
            // the node (r, c) and centre (r, c) terms are shared by the u and v rows: the v row's are -tn (the same
            // differences negated: exact) and tc (the same sum, operands swapped: exact)
            const double tn = (uN - uC) + (vC - vW), tc = (uE - uC) + (vS - vC);
            // u row: v1 = vW, v2 = vC, v3 = vSW, v4 = vS
            double br = KC * tn;
            br = __builtin_fma(A1, (uW - uC) + (vW - vSW), br);
            br = __builtin_fma(A2, tc, br);
            br = __builtin_fma(KS, (uS - uC) + (vSW - vS), br);
            acc[fu] = __builtin_fma(a, br, __builtin_fma(w.wu[p], uC, p ? -xdu : xdu));
            // v row: u1 = uN, u2 = uNE, u3 = uC, u4 = uE
            double bv = B1 * ((vN - vC) + (uN - uNE));
            bv = __builtin_fma(KC, -tn, bv);
            bv = __builtin_fma(KE, (vE - vC) + (uNE - uE), bv);
            bv = __builtin_fma(A2, tc, bv);
            acc[fv] = __builtin_fma(a, bv, __builtin_fma(w.wv[p], vC, p ? -xdv : xdv));
        }
    }
    // the four rows (u_n, v_n, u_s, v_s) of cell (gr, gc) and their reciprocal diagonals
    // RD = false: the diagonals are the caller's (k_ftile level B reuses level A's, computed by the same operations)
    template <bool RD = true, class TA, class XA>
    __device__ void rows4(int gr, int gc, const TA& ta, const XA& xa, const Cell& cl, double* acc, double* rd) const {
        const Co k = coeffs(nb(ta, gr, gc));
        const W4 w = weights(cl);
        rows4_co(gr, gc, k, w, xa, acc);
        if constexpr (RD) rdiag4_co(k, w, rd);
    }
    // the reciprocal diagonals from a cell's coefficients and weights (rdiag4's arithmetic)
    __device__ void rdiag4_co(const Co& k, const W4& w, double* rd) const {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            auto ph = [&](double t) { return p ? 1.0 - t : t; };
            const double a = aco(p);
            const double A1 = ph(k.w), A2 = ph(k.c), B1 = ph(k.nn), KC = ph(k.kc), KS = ph(k.ks), KE = ph(k.ke);
            rd[2 * p] = rcp_nr(__builtin_fma(-a, (A1 + A2) + (KC + KS), w.wu[p] + k.xu));
            rd[2 * p + 1] = rcp_nr(__builtin_fma(-a, (B1 + A2) + (KC + KE), w.wv[p] + k.xv));
        }
    }
    // the reciprocal diagonals of the four rows at a staged point (k_march_init: x0 = c2 b / diag)
    template <class TA>
    __device__ void rdiag4(int gr, int gc, const TA& ta, const Stage& sg, double* rd) const {
        const Co k = coeffs(nb(ta, gr, gc));
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            auto ph = [&](double t) { return p ? 1.0 - t : t; };
            const double a = aco(p);
            const double A1 = ph(k.w), A2 = ph(k.c), B1 = ph(k.nn), KC = ph(k.kc), KS = ph(k.ks), KE = ph(k.ke);
            rd[2 * p] = rcp_nr(__builtin_fma(-a, (A1 + A2) + (KC + KS), c * ph(sg.face[0]) + k.xu));
            rd[2 * p + 1] = rcp_nr(__builtin_fma(-a, (B1 + A2) + (KC + KE), c * ph(sg.face[1]) + k.xv));
        }
    }
};

// Tolerance-mode F inner solve from x = 0 on a row partition's owned rows (the per-operator exchange schedule: the
// multigrid level-0 smoothing and the Chebyshev / Jacobi F solves there): x0 = d0 = (c2 b) (1 / diag) with the
// reciprocal diagonals of FStencilFast::rdiag4 over the global thn table -- the operations of the one-GPU fast first
// sweep (k_ftile / k_fsolve level 0, k_march_init), so the partitioned fast solve starts from the same bits (the stored
// diagonal's c2 (b / diag) does not).  One thread per owned cell, its four rows.
struct TGlob {   // thn at wrapped grid coordinates, straight from the global table
    const double* t;
    int n;
    __device__ double T(int sph, int r, int c) const {
        r = r < 0 ? r + n : (r >= n ? r - n : r);
        c = c < 0 ? c + n : (c >= n ? c - n : c);
        const double v = t[r * n + c];
        return sph ? 1.0 - v : v;
    }
};
template <bool CHEB>
__global__ void __launch_bounds__(256) k_f_fast_init(FStencilFast P, const double* __restrict__ b, double c2,
                                                     double* __restrict__ d, const double* __restrict__ sub,
                                                     double* __restrict__ xo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)P.L * P.n) return;
    const int lr = (int)(i / P.n), gc = (int)(i - (int64_t)lr * P.n);
    const int gr = P.r0 + lr;
    const int32_t k = gr * P.n + gc;
    const FStencilDev::Stage sg{{P.uface[k], P.vface[k]}};
    double rd[4];
    P.rdiag4(gr, gc, TGlob{P.cell, P.n}, sg, rd);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int64_t o = ((int64_t)f * P.L + lr) * P.n + gc;
        const double x0 = c2 * b[o] * rd[f];
        if constexpr (CHEB) d[o] = x0;
        xo[o] = sub ? sub[o] - x0 : x0;
    }
}

// ---- marching kernels: a workgroup owns a 256-column strip of `rows` consecutive grid rows and walks
// down it with a 3-row LDS ring per staged field (+ thn).  Each step stages ONE new grid row (its loads
// are issued before the current row is computed, so their latency hides under the arithmetic) instead
// of three, and the epilogue operands of the row are requested before the barrier.  The kernel is
// generic over the stencil S (F, D, G, Gt_G below):
//   S::NF staged input fields, S::NOUT output rows per cell, S::xrow(f, gr) the input layout,
//   S::out_row(o, lr, gc) the output layout, S::row<EDGE>(o, ...) output row o's sum and diagonal
//   (EDGE: the cell is on the grid's border, where periodic wrap reorders the row's columns);
// and over the source XS of the staged input: the vector itself, or (first inner sweep) the inner
// solver's x0 = c2 * (b / diag) recomputed from b and diag, so that sweep needs no init pass.
constexpr int kMB = 256;   // columns (threads) per marching workgroup
constexpr int kMTileW = kMB + 2;       // + one halo column each side
struct XRing {
    const double* x;   // [NF][3][kMTileW]
    int s[3];          // ring slot of rows gr-1, gr, gr+1
    int gr, c0;
    __device__ double X(int f, int r, int c) const { return x[(f * 3 + s[r - gr + 1]) * kMTileW + (c - c0 + 1)]; }
};
template <int W, int OFF>
struct TRingT {
    const double* t;   // [slots][W]: tile column 0 is grid column c0 - OFF
    int s[3];
    int gr, c0;
    __device__ double T(int sph, int r, int c) const {
        const double v = t[s[r - gr + 1] * W + (c - c0 + OFF)];
        return sph ? 1.0 - v : v;
    }
};
using TRing = TRingT<kMTileW, 1>;

// Staged sources: load(i) issues the loads of element i (raw registers, nothing consumes them yet), value(raw)
// turns them into the staged value at LDS-store time -- so a tile row's loads stay in flight through the
// previous row's compute even when the staged value needs arithmetic (XInit's division).
struct XPlain {        // staged value = x[i]
    const double* __restrict__ x;
    typedef double Raw;
    __device__ Raw load(int32_t i) const { return x[i]; }
    __device__ double value(const Raw& r) const { return r; }
    __device__ double operator()(int32_t i) const { return x[i]; }
};
struct XInitRaw {
    double b, d;
};
struct XInit {         // staged value = the first inner iterate: c2 * (b[i] / diag[i]) (c2 = 1: Jacobi)
    const double* __restrict__ b;
    const double* __restrict__ dg;
    double c2;
    typedef XInitRaw Raw;
    __device__ Raw load(int32_t i) const { return {b[i], dg[i]}; }
    __device__ double value(const Raw& r) const { return c2 * (r.b / r.d); }
    __device__ double operator()(int32_t i) const { return c2 * (b[i] / dg[i]); }
};

// Right-hand-side sources of the marching F sweeps.  BNone: the epilogue loads b.  GxB: b is the velocity row of
// W = G x_p (solve.py:273), recomputed per row from x_p and the staged cell thn with GStencilDev::row's arithmetic
// (d_p, 1/dx, -1/dx and the wrapped neighbour's position exactly as there), so the second F solve of the apply
// (solve.py:274) reads one pressure field (8 B per cell, cached neighbours) instead of W's four (32 B per cell),
// and W is never written.  One GPU (whole-grid layouts).
struct BNone {
    static constexpr bool on = false, part = false, resid = false;
    struct Q {};
    __device__ Q load(int, int, int) const { return {}; }
    template <class TA>
    __device__ double b(int, int, int, int, const TA&, const Q&) const { return 0.0; }
};
// PART: x_p in a row partition's ghost layout (L owned rows, h ghost rows each side); else the whole grid.
template <bool PART>
struct GxBT {
    static constexpr bool on = true, part = PART, resid = false;
    const double* __restrict__ xp;
    double d_p, inv, minv;
    int n;
    int L = 0, h = 0;
    struct Q { double c, w, nn; };   // x_p at the cell and at its west and north neighbours (periodic)
    __device__ int32_t row(int lr, int gr) const { return PART ? ext_row(1, 0, lr, L, h, n) : gr * n; }
    // lr: the cell's local row in the partition layout, (gr, gc): its wrapped global grid coordinates
    __device__ Q load(int lr, int gr, int gc) const {
        const int gw = gc == 0 ? n - 1 : gc - 1, gn = gr == 0 ? n - 1 : gr - 1;
        const int32_t rc = row(lr, gr), rn = row(lr - 1, gn);
        return {xp[rc + gc], xp[rc + gw], xp[rn + gc]};
    }
    // velocity row o (u_n, v_n, u_s, v_s) at the cell: TA::T(p, r, c) in the accessor's coordinates (gr, c), the
    // cell's wrapped column gc decides the periodic order as GStencilDev::row does
    template <class TA>
    __device__ double b(int o, int gr, int c, int gc, const TA& ta, const Q& q) const {
        return b_at(o, gr, c, gc == 0, gr == 0, ta, q);
    }
    // the same with ta at coordinates (r, c) of the accessor's own and the cell's periodic position given as flags:
    // wrapw, its grid column is 0 (its west neighbour wraps); wrapn, its grid row is 0
    template <class TA>
    __device__ double b_at(int o, int r, int c, bool wrapw, bool wrapn, const TA& ta, const Q& q) const {
        const int p = o >> 1;
        const double t0 = ta.T(p, r, c);
        double acc = 0.0;
        if ((o & 1) == 0) {   // u row: entries p(gr, gc-1), p(gr, gc); the wrapped one sorts last
            const double gu = 0.5 * (t0 + ta.T(p, r, c - 1));
            const double uC = (d_p * (inv * gu)) * q.c, uW = (d_p * (minv * gu)) * q.w;
            acc += wrapw ? uC : uW;
            acc += wrapw ? uW : uC;
        } else {              // v row: entries p(gr-1, gc), p(gr, gc)
            const double gv = 0.5 * (t0 + ta.T(p, r - 1, c));
            const double vC = (d_p * (minv * gv)) * q.c, vN = (d_p * (inv * gv)) * q.nn;
            acc += wrapn ? vC : vN;
            acc += wrapn ? vN : vC;
        }
        return acc;
    }
};
using GxB = GxBT<false>;
using GxBPart = GxBT<true>;
// GxR: b = z - G x_p, the right-hand side of the upper block form's one F solve (u = F^-1 (v_u - G x_p),
// mpbp_schur_plan.form): GxB's row of G x_p (b_at: the same products in the same periodic order), then the one
// subtraction EpiResid makes of it -- the bits of the G launch in MPBP_SPMV_RESID mode, W never stored.  The whole-solve
// launches only (k_fsolve_w, k_fsolve): they stage x_p as for GxB and load z per owned cell where BNone loads b.
struct GxR : GxBT<false> {
    static constexpr bool resid = true;
    const double* __restrict__ z;
};

// Row of tile values held between its loads and its LDS store: every lane's main column (xa, ta; tile columns
// c0-1 .. c0+254) and (lanes 0, 1) the halo columns c0+255, c0+256 (h0, t0).  (Holding the halo columns in SGPRs
// through scalar loads measured slower)
template <int NF, class Raw>
struct TileRow {
    Raw xa[NF], h0[NF];
    double ta, t0;
};

// Columns of the strip's right-hand halo (tile columns kMB, kMB + 1) and whether they exist.
struct HaloCols {
    int g0, g1;     // wrapped grid columns
    bool ok0, ok1;  // inside the grid or its periodic right neighbour (column n -> 0)
    int gl;         // this lane's halo column (lanes 0, 1: g0, g1; others re-read their main column, cached)
};

template <class S, class XS>
__device__ inline void load_tile_row(const S& P, const XS& xs, int gr, int gcA, bool okA, const HaloCols& hc,
                                     TileRow<S::NF, typename XS::Raw>& tr) {
    // Every load unconditional (lanes without a column of their own read a clamped one): no branch around a
    // load, so the compiler's wait counts stay exact and the row's loads remain in flight through the next
    // compute.  The selects happen at the LDS store (store_tile_row).
    const int ca = okA ? gcA : 0;
#pragma unroll
    for (int f = 0; f < S::NF; ++f) {
        const int32_t base = P.xrow(f, gr);
        tr.xa[f] = xs.load(base + ca);
        tr.h0[f] = xs.load(base + hc.gl);
    }
    const int32_t tb = P.wrap(gr) * P.n;
    tr.ta = P.cell[tb + ca];
    tr.t0 = P.cell[tb + hc.gl];
}

template <class XS, int NF>
__device__ inline void store_tile_row(const XS& xs, double* sx, double* st, int slot, int tid, bool okA,
                                      const HaloCols& hc, const TileRow<NF, typename XS::Raw>& tr) {
#pragma unroll
    for (int f = 0; f < NF; ++f) sx[(f * 3 + slot) * kMTileW + tid] = okA ? xs.value(tr.xa[f]) : 0.0;
    st[slot * kMTileW + tid] = okA ? tr.ta : 0.0;
    if (tid < 2) {   // lanes 0 and 1 store the halo columns
        const bool ok = tid == 0 ? hc.ok0 : hc.ok1;
#pragma unroll
        for (int f = 0; f < NF; ++f) sx[(f * 3 + slot) * kMTileW + kMB + tid] = ok ? xs.value(tr.h0[f]) : 0.0;
        st[slot * kMTileW + kMB + tid] = ok ? tr.t0 : 0.0;
    }
}

// Grid rows [la, lb) of workgroup chunk `chunk` of `nchunks`: which = 0 all owned rows, 1 rows 1 .. L-2 (no
// ghost read), 2 rows 0 and L-1 (one chunk each), 3 the owned rows and `ext` ghost rows each side.  The
// rows are split evenly (chunk sizes differ by at most one), so a launch can be sized to one round of
// workgroups (launch_march).
__device__ inline bool march_rows(int which, int L, int ext, int chunk, int nchunks, int* la, int* lb) {
    if (which == 2) {
        *la = chunk == 0 ? 0 : L - 1;
        *lb = *la + 1;
        return chunk < (L >= 2 ? 2 : 1);
    }
    const int lo = which == 1 ? 1 : which == 3 ? -ext : 0;
    const int hi = which == 1 ? L - 1 : which == 3 ? L + ext : L;
    const int rows = hi - lo;
    *la = lo + (int)((int64_t)chunk * rows / nchunks);
    *lb = lo + (int)((int64_t)(chunk + 1) * rows / nchunks);
    return *la < *lb;
}

template <class S, class XS, class Epi, class BS = BNone>
// (4 waves per SIMD asked for explicitly: the F Chebyshev instance would otherwise take 130 VGPRs -> 3)
__global__ void __launch_bounds__(kMB) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_march(S P, XS xs, int nchunks, Epi epi, BS bs = BS{}) {
    constexpr int NF = S::NF, NO = S::NOUT;
    static_assert(!S::kFast || RcpOk<Epi>::value, "a tolerance-mode policy hands over reciprocal diagonals");
    __shared__ double sx[NF * 3 * kMTileW];
    __shared__ double st[3 * kMTileW];
    const int n = P.n;
    const int strips = (n + kMB - 1) / kMB;
    const int b = xcd_swizzle(blockIdx.x, gridDim.x);
    const int strip = b % strips, chunk = b / strips;
    int la, lb;
    if (!march_rows(P.which, P.L, P.ext, chunk, nchunks, &la, &lb)) return;
    const int c0 = strip * kMB, tid = threadIdx.x;
    const int colA = c0 - 1 + tid;
    const bool okA = colA <= n;
    const int gcA = P.wrap(colA);
    // the right-hand halo columns c0+255, c0+256 (the grid's last column's periodic neighbour is column 0)
    HaloCols hc;
    {
        const int b0 = c0 + kMB - 1, b1 = c0 + kMB;
        hc.ok0 = b0 <= n;
        hc.ok1 = b1 <= n;
        hc.g0 = b0 < n ? b0 : 0;
        hc.g1 = b1 < n ? b1 : 0;
        hc.gl = tid == 0 ? hc.g0 : tid == 1 ? hc.g1 : (okA ? gcA : 0);
    }
    const int gc = c0 + tid;
    const bool live = gc < n;
    // prologue: rows la-1 -> slot 0, la -> slot 1; row la+1 in registers -- all three requested at once
    typedef TileRow<NF, typename XS::Raw> TR;
    TR tr, tp0, tp1;
    load_tile_row(P, xs, P.r0 + la - 1, gcA, okA, hc, tp0);
    load_tile_row(P, xs, P.r0 + la, gcA, okA, hc, tp1);
    load_tile_row(P, xs, P.r0 + la + 1, gcA, okA, hc, tr);
    store_tile_row(xs, sx, st, 0, tid, okA, hc, tp0);
    store_tile_row(xs, sx, st, 1, tid, okA, hc, tp1);
    // One step: row lr+1 into the ring, the next row's loads issued (LOAD: every step but the last, which is
    // peeled off so that no load sits under a branch), row lr computed from LDS.
    auto step = [&](int lr, auto load_next) {
        const int k = lr - la;
        const int sm = k % 3, s0 = (k + 1) % 3, sp = (k + 2) % 3;
        store_tile_row(xs, sx, st, sp, tid, okA, hc, tr);   // row lr+1
        // operands of this row's epilogues and cells, requested unconditionally (lanes past the grid edge
        // read row 0 and discard it) so the wait counts stay exact and later loads stay in flight
        const int gcl = live ? gc : 0;
        typename Epi::P pe[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) pe[o] = epi.pre_lite(P.out_row(o, lr, gcl));
        const typename S::Cell cl = P.cell_pre(P.wrap(P.r0 + lr), gcl);   // ghost rows wrap periodically
        const typename BS::Q bq = bs.load(lr, P.wrap(P.r0 + lr), gcl);
        __syncthreads();
        if constexpr (decltype(load_next)::value) load_tile_row(P, xs, P.r0 + lr + 2, gcA, okA, hc, tr);
        if (live) {
            const int gr = P.wrap(P.r0 + lr);
            const XRing xa{sx, {sm, s0, sp}, gr, c0};
            const TRing ta{st, {sm, s0, sp}, gr, c0};
            if constexpr (S::kFast) {   // tolerance mode: the cell's rows at once, reciprocal diagonals
                double acc[NO], rd[NO];
                P.rows4(gr, gc, ta, xa, cl, acc, rd);
                if constexpr (CellEpi<Epi>::value) {   // (the reciprocal diagonals are not used)
                    double xv[NO];
                    int32_t rw[NO];
#pragma unroll
                    for (int o = 0; o < NO; ++o) {
                        xv[o] = xa.X(o, gr, gc);
                        rw[o] = P.out_row(o, lr, gc);
                    }
                    epi.cell(rw, acc, xv, pe);
                } else {
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    set_diag(pe[o], rd[o]);
                    set_x(pe[o], xa.X(o, gr, gc));
                    if constexpr (BS::on) set_b(pe[o], bs.b(o, gr, gc, gc, ta, bq));
                    epi(P.out_row(o, lr, gc), acc[o], pe[o]);
                }
                }
            } else {
            // the wrap-aware (sorting) form is exact for interior cells too: take it for the whole wave when
            // any of its cells is on the periodic edge, so a wave never runs both forms
            const bool edge = __builtin_amdgcn_readfirstlane(__any(gr == 0 || gr == n - 1 || gc == 0 || gc == n - 1)) != 0;
            if constexpr (CellEpi<Epi>::value) {   // the cell's row sums (row<EDGE>'s bits), then the rows together
                double acc[NO], xv[NO];
                int32_t rw[NO];
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    double dg;
                    acc[o] = edge ? P.template row<true>(o, gr, gc, ta, xa, &dg, cl)
                                  : P.template row<false>(o, gr, gc, ta, xa, &dg, cl);
                    xv[o] = xa.X(S::NF == 1 ? 0 : o, gr, gc);
                    rw[o] = P.out_row(o, lr, gc);
                }
                epi.cell(rw, acc, xv, pe);
            } else {
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                double dg;
                const double acc = edge ? P.template row<true>(o, gr, gc, ta, xa, &dg, cl)
                                        : P.template row<false>(o, gr, gc, ta, xa, &dg, cl);
                set_diag(pe[o], dg);
                set_x(pe[o], xa.X(S::NF == 1 ? 0 : o, gr, gc));
                if constexpr (BS::on) set_b(pe[o], bs.b(o, gr, gc, gc, ta, bq));
                epi(P.out_row(o, lr, gc), acc, pe[o]);
            }
            }
            }
        }
        __syncthreads();                                     // slot sm is rewritten next step
    };
    for (int lr = la; lr < lb - 1; ++lr) step(lr, std::true_type{});
    step(lb - 1, std::false_type{});
}

// ---- direct kernel for the pressure-side stencils (D, G, Gt_G) ----
// One thread per cell, no LDS and no barrier: the stencil reads its neighbours straight from global memory (the
// 8 MB pressure vectors and the thn table stay L2-resident), so a launch is n^2 / 256 independent workgroups at
// full occupancy instead of one round of marching workgroups.  Same accessors' values, same row arithmetic.
// Measured at 1024^2 (trace means, r02o vs r02l): D 17.7 -> 13.2 us, Gt_G sweeps 13.2 / 12.1 -> 11.9 / 11.3 us, the
// Gt_G first sweep (5 divisions per cell for the staged x0) 15.6 either way.
// (lr: the thread's local row in the partition layout, gr: the same row's wrapped global index -- the row the
// stencil's accessors are called around; a neighbour row r maps to local row lr + (r - gr))
template <class S, class XS>
struct XDirect {
    const S& P;
    const XS& xs;
    int lr, gr;
    __device__ double X(int f, int r, int c) const { return xs(P.xrow(f, P.r0 + lr + (r - gr)) + P.wrap(c)); }
};
struct TDirect {
    const double* __restrict__ cell;
    int n;
    __device__ double T(int sph, int r, int c) const {
        const int rr = r < 0 ? r + n : (r >= n ? r - n : r), cc = c < 0 ? c + n : (c >= n ? c - n : c);
        const double v = cell[rr * n + cc];
        return sph ? 1.0 - v : v;
    }
};
// Rows [la, la + rows) of the partition (which = 2: rows 0 and L - 1), one thread per (row, column).
template <class S, class XS, class Epi, class BS = BNone>
__global__ void __launch_bounds__(256) k_direct(S P, XS xs, Epi epi, int la, int rows, BS bs = BS{}) {
    constexpr int NO = S::NOUT;
    static_assert(!S::kFast || RcpOk<Epi>::value, "a tolerance-mode policy hands over reciprocal diagonals");
    const int n = P.n;
    const int64_t t = (int64_t)xcd_swizzle(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    const bool live = t < (int64_t)rows * n;
    const int tt = live ? (int)t : 0;
    const int li = tt / n, gc = tt - li * n;
    const int lr = P.which == 2 ? (li == 0 ? 0 : P.L - 1) : la + li;
    const int gr = P.wrap(P.r0 + lr);
    typename Epi::P pe[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) pe[o] = epi.pre_lite(P.out_row(o, lr, gc));
    const typename S::Cell cl = P.cell_pre(gr, gc);
    const XDirect<S, XS> xa{P, xs, lr, gr};
    const TDirect ta{P.cell, n};
    const typename BS::Q bq = bs.load(lr, gr, gc);
    if constexpr (S::kFast) {   // tolerance-mode F: the cell's four rows at once, reciprocal diagonals
        if (!live) return;
        double acc[NO], rd[NO];
        P.rows4(gr, gc, ta, xa, cl, acc, rd);
        if constexpr (CellEpi<Epi>::value) {   // (the reciprocal diagonals are not used)
            double xv[NO];
            int32_t rw[NO];
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                xv[o] = xa.X(o, gr, gc);
                rw[o] = P.out_row(o, lr, gc);
            }
            epi.cell(rw, acc, xv, pe);
        } else {
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            set_diag(pe[o], rd[o]);
            set_x(pe[o], xa.X(o, gr, gc));
            if constexpr (BS::on) set_b(pe[o], bs.b(o, gr, gc, gc, ta, bq));
            epi(P.out_row(o, lr, gc), acc[o], pe[o]);
        }
        }
        return;
    }
    if constexpr (!CellEpi<Epi>::value) {   // (a cell-wise epilogue reaches k_direct through the tolerance-mode F rows only)
    const bool edge = __builtin_amdgcn_readfirstlane(__any(gr == 0 || gr == n - 1 || gc == 0 || gc == n - 1)) != 0;
    if (!live) return;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        double dg;
        const double acc = edge ? P.template row<true>(o, gr, gc, ta, xa, &dg, cl)
                                : P.template row<false>(o, gr, gc, ta, xa, &dg, cl);
        set_diag(pe[o], dg);
        set_x(pe[o], xa.X(S::NF == 1 ? 0 : o, gr, gc));
        epi(P.out_row(o, lr, gc), acc, pe[o]);
    }
    }
}

// ---- first inner sweep with the init pass folded in, diagonal recomputed (k_march_init) ----
// The sweep stages x0 = c2 * (b / diag) (c2 = 1: Jacobi) wherever k_march would stage x, with diag -- the
// operator's own diagonal at the staged point -- rebuilt from the thn tile by the stencil (S::stage_diag, the
// same expression its rows use), so the sweep streams b alone: no diag vector, and one value in flight per
// staged point.  Rebuilding the staged row's diagonal needs thn one row below it, so the thn ring runs a row
// ahead of the x ring: 5 slots over columns c0-2 .. c0+257 (one more each side than the x tile, for the v
// rows' and the halo columns' neighbours).  Invariant at the start of step k: thn rows k-1 .. k+2 and x0 rows
// k-1, k in LDS, b row k+1 (+ its S::Stage operands) in registers.
constexpr int kTW = kMTileW + 2;
template <int NF, class Stage, class BS = BNone>
struct InitRow {
    double xa[NF], h0[NF];   // b at the lane's main column and (lanes 0, 1) its halo column
    Stage sa, sh;            // the stencil's per-point operands for the diagonal (F: the u/v face thn)
};
template <int NF, class Stage, bool PT>
struct InitRow<NF, Stage, GxBT<PT>> {
    typename GxBT<PT>::Q qa, qh;   // b recomputed from x_p (GxB): its operands at the main and the halo column
    Stage sa, sh;
};
struct ThnRow {
    double ta, te;           // thn at the lane's main column; lanes 0..3 an extra column (c0+255, c0+256, c0-2, c0+257)
};
__device__ inline int thn_extra_col(int tid, int c0) {
    return tid == 0 ? c0 + kMB - 1 : tid == 1 ? c0 + kMB : tid == 2 ? c0 - 2 : c0 + kMB + 1;
}
__device__ inline int thn_extra_slot(int tid) { return tid == 0 ? kMB + 1 : tid == 1 ? kMB + 2 : tid == 2 ? 0 : kMB + 3; }

template <class S>
__device__ inline void load_thn_row(const S& P, int gr, int colA, int tid, int c0, ThnRow& t) {
    const int n = P.n;
    const int32_t tb = P.wrap(gr) * n;
    const int ce = thn_extra_col(tid, c0);
    t.ta = P.cell[tb + (colA <= n + 1 ? P.wrap(colA) : 0)];
    t.te = P.cell[tb + (ce <= n + 1 ? P.wrap(ce) : 0)];
}
__device__ inline void store_thn_row(double* st, int slot, int tid, const ThnRow& t) {
    st[slot * kTW + tid + 1] = t.ta;
    if (tid < 4) st[slot * kTW + thn_extra_slot(tid)] = t.te;
}
template <class S, class BS>
__device__ inline void load_init_row(const S& P, const double* __restrict__ b, int gr, int gcA, bool okA,
                                     const HaloCols& hc, InitRow<S::NF, typename S::Stage, BS>& tr, const BS& bs) {
    const int ca = okA ? gcA : 0;
    if constexpr (BS::on) {   // (gr: the unwrapped global row; its local row is gr - r0)
        tr.qa = bs.load(gr - P.r0, P.wrap(gr), ca);
        tr.qh = bs.load(gr - P.r0, P.wrap(gr), hc.gl);
    } else {
#pragma unroll
        for (int f = 0; f < S::NF; ++f) {
            const int32_t base = P.xrow(f, gr);
            tr.xa[f] = b[base + ca];
            tr.h0[f] = b[base + hc.gl];
        }
    }
    tr.sa = P.stage_pre(gr, ca);
    tr.sh = P.stage_pre(gr, hc.gl);
}
// x0 of staged grid row gr (ring slot `slot`) from b and the diagonal rebuilt over thn rows gr-1 .. gr+1.
template <class S, class BS>
__device__ inline void store_init_row(const S& P, double c2, double* sx, const double* st, int slot, const int ts[3],
                                      int gr, int c0, int tid, int colA, bool okA, const HaloCols& hc,
                                      const InitRow<S::NF, typename S::Stage, BS>& tr, const BS& bs) {
    const TRingT<kTW, 2> ta{st, {ts[0], ts[1], ts[2]}, gr, c0};
    if constexpr (S::kFast) {   // tolerance mode: x0 = c2 b (1 / diag), the four reciprocal diagonals at once
        double rd[4];
        P.rdiag4(gr, colA, ta, tr.sa, rd);
#pragma unroll
        for (int f = 0; f < S::NF; ++f) {
            double bf;
            if constexpr (BS::on) bf = bs.b(f, gr, colA, P.wrap(colA), ta, tr.qa);
            else bf = tr.xa[f];
            sx[(f * 3 + slot) * kMTileW + tid] = okA ? c2 * bf * rd[f] : 0.0;
        }
        if (tid < 2) {
            const bool ok = tid == 0 ? hc.ok0 : hc.ok1;
            const int col = c0 + kMB - 1 + tid;
            P.rdiag4(gr, col, ta, tr.sh, rd);
#pragma unroll
            for (int f = 0; f < S::NF; ++f) {
                double bf;
                if constexpr (BS::on) bf = bs.b(f, gr, col, P.wrap(col), ta, tr.qh);
                else bf = tr.h0[f];
                sx[(f * 3 + slot) * kMTileW + kMB + tid] = ok ? c2 * bf * rd[f] : 0.0;
            }
        }
        return;
    }
#pragma unroll
    for (int f = 0; f < S::NF; ++f) {
        const double dg = P.stage_diag(f, gr, colA, ta, tr.sa);
        double bf;
        if constexpr (BS::on) bf = bs.b(f, gr, colA, P.wrap(colA), ta, tr.qa);
        else bf = tr.xa[f];
        sx[(f * 3 + slot) * kMTileW + tid] = okA ? c2 * (bf / dg) : 0.0;
    }
    if (tid < 2) {   // lanes 0 and 1: the halo columns c0+255, c0+256
        const bool ok = tid == 0 ? hc.ok0 : hc.ok1;
        const int col = c0 + kMB - 1 + tid;
#pragma unroll
        for (int f = 0; f < S::NF; ++f) {
            const double dg = P.stage_diag(f, gr, col, ta, tr.sh);
            double bf;
            if constexpr (BS::on) bf = bs.b(f, gr, col, P.wrap(col), ta, tr.qh);
            else bf = tr.h0[f];
            sx[(f * 3 + slot) * kMTileW + kMB + tid] = ok ? c2 * (bf / dg) : 0.0;
        }
    }
}

template <class S, class Epi, class BS = BNone>
__global__ void __launch_bounds__(kMB) __attribute__((amdgpu_waves_per_eu(4, 8)))
k_march_init(S P, const double* __restrict__ b, double c2, int nchunks, Epi epi, BS bs = BS{}) {
    constexpr int NF = S::NF, NO = S::NOUT;
    static_assert(!S::kFast || RcpOk<Epi>::value, "a tolerance-mode policy hands over reciprocal diagonals");
    __shared__ double sx[NF * 3 * kMTileW];
    __shared__ double st[5 * kTW];
    const int n = P.n;
    const int strips = (n + kMB - 1) / kMB;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int strip = bk % strips, chunk = bk / strips;
    int la, lb;
    if (!march_rows(P.which, P.L, P.ext, chunk, nchunks, &la, &lb)) return;
    const int c0 = strip * kMB, tid = threadIdx.x;
    const int colA = c0 - 1 + tid;
    const bool okA = colA <= n;
    const int gcA = P.wrap(colA <= n + 1 ? colA : 0);
    HaloCols hc;
    {
        const int b0 = c0 + kMB - 1, b1 = c0 + kMB;
        hc.ok0 = b0 <= n;
        hc.ok1 = b1 <= n;
        hc.g0 = b0 < n ? b0 : 0;
        hc.g1 = b1 < n ? b1 : 0;
        hc.gl = tid == 0 ? hc.g0 : tid == 1 ? hc.g1 : (okA ? gcA : 0);
    }
    const int gc = c0 + tid;
    const bool live = gc < n;
    auto tslot = [&](int lr) { return (lr - la + 2) % 5; };   // thn ring slot of local row lr (lr >= la - 2)
    auto xslot = [&](int lr) { return (lr - la + 1) % 3; };   // x ring slot (lr >= la - 1)
    auto grow = [&](int lr) { return P.wrap(P.r0 + lr); };    // grid row (ghost rows wrap periodically)
    typedef InitRow<NF, typename S::Stage, BS> IR;
    // prologue: thn rows la-2 .. la+2, x0 rows la-1 and la; b row la+1 into registers
    {
        ThnRow t[5];
        IR r0, r1;
#pragma unroll
        for (int i = 0; i < 5; ++i) load_thn_row(P, P.r0 + la - 2 + i, colA, tid, c0, t[i]);
        load_init_row(P, b, P.r0 + la - 1, gcA, okA, hc, r0, bs);
        load_init_row(P, b, P.r0 + la, gcA, okA, hc, r1, bs);
#pragma unroll
        for (int i = 0; i < 5; ++i) store_thn_row(st, i, tid, t[i]);
        __syncthreads();
        const int s0[3] = {tslot(la - 2), tslot(la - 1), tslot(la)};
        store_init_row(P, c2, sx, st, xslot(la - 1), s0, grow(la - 1), c0, tid, colA, okA, hc, r0, bs);
        const int s1[3] = {tslot(la - 1), tslot(la), tslot(la + 1)};
        store_init_row(P, c2, sx, st, xslot(la), s1, grow(la), c0, tid, colA, okA, hc, r1, bs);
    }
    IR tr;
    ThnRow tn;
    load_init_row(P, b, P.r0 + la + 1, gcA, okA, hc, tr, bs);
    auto step = [&](int lr, auto load_next) {
        {   // x0 of row lr+1 (thn rows lr .. lr+2)
            const int ts[3] = {tslot(lr), tslot(lr + 1), tslot(lr + 2)};
            store_init_row(P, c2, sx, st, xslot(lr + 1), ts, grow(lr + 1), c0, tid, colA, okA, hc, tr, bs);
        }
        const int gcl = live ? gc : 0;
        typename Epi::P pe[NO];
#pragma unroll
        for (int o = 0; o < NO; ++o) pe[o] = epi.pre_lite(P.out_row(o, lr, gcl));
        const typename S::Cell cl = P.cell_pre(grow(lr), gcl);
        const typename BS::Q bq = bs.load(lr, grow(lr), gcl);
        __syncthreads();
        if constexpr (decltype(load_next)::value) {   // thn row lr+3 first: it is stored at the end of this step
            load_thn_row(P, P.r0 + lr + 3, colA, tid, c0, tn);
            load_init_row(P, b, P.r0 + lr + 2, gcA, okA, hc, tr, bs);
        }
        if constexpr (S::kFast) if (live) {
            const int gr = grow(lr);
            const XRing xa{sx, {xslot(lr - 1), xslot(lr), xslot(lr + 1)}, gr, c0};
            const TRingT<kTW, 2> ta{st, {tslot(lr - 1), tslot(lr), tslot(lr + 1)}, gr, c0};
            double acc[NO], rd[NO];
            P.rows4(gr, gc, ta, xa, cl, acc, rd);
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                set_diag(pe[o], rd[o]);
                set_x(pe[o], xa.X(o, gr, gc));
                if constexpr (BS::on) set_b(pe[o], bs.b(o, gr, gc, gc, ta, bq));
                epi(P.out_row(o, lr, gc), acc[o], pe[o]);
            }
        }
        if constexpr (!S::kFast) if (live) {
            const int gr = grow(lr);
            const XRing xa{sx, {xslot(lr - 1), xslot(lr), xslot(lr + 1)}, gr, c0};
            const TRingT<kTW, 2> ta{st, {tslot(lr - 1), tslot(lr), tslot(lr + 1)}, gr, c0};
            const bool edge = __builtin_amdgcn_readfirstlane(__any(gr == 0 || gr == n - 1 || gc == 0 || gc == n - 1)) != 0;
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                double dg;
                const double acc = edge ? P.template row<true>(o, gr, gc, ta, xa, &dg, cl)
                                        : P.template row<false>(o, gr, gc, ta, xa, &dg, cl);
                set_diag(pe[o], dg);
                set_x(pe[o], xa.X(S::NF == 1 ? 0 : o, gr, gc));
                if constexpr (BS::on) set_b(pe[o], bs.b(o, gr, gc, gc, ta, bq));
                epi(P.out_row(o, lr, gc), acc, pe[o]);
            }
        }
        if constexpr (decltype(load_next)::value) store_thn_row(st, tslot(lr + 3), tid, tn);   // slot of row lr-2
        __syncthreads();
    };
    for (int lr = la; lr < lb - 1; ++lr) step(lr, std::true_type{});
    step(lb - 1, std::false_type{});
}

// ---- two fused Chebyshev sweeps over F, tolerance mode (k_march2) ----
// Sweeps s and s+1 of an F Chebyshev solve in one pass down the strip.  Level A stages x_{s-1} (x_in) in a 3-row
// LDS ring and computes x_s, d_s of grid row t; x_s goes to a second ring, d_s (and b, the faces) stay in the lane's
// registers -- level B, one row behind, computes x_{s+1} of row t-1 on the same column from that ring.  Per F row the
// pair reads x_in, d_in, b (or x_p, GxB), thn and writes x_out (+ d_out unless the pair ends the solve): 38 B instead of
// 84 B for two k_march sweeps; x_s and d_s never leave the CU.  Level A also computes x_s on the columns either side
// of the strip (c0 - 1, c0 + 256: one extra pass of lanes 0, 1) for level B's stencil.  Each level performs exactly
// the IEEE operations of one tolerance-mode k_march sweep (FStencilFast::rows4, the RCP Chebyshev update), so the pair
// is bit-identical to two k_march sweeps.  Rows: level A [la-1, lb], level B [la, lb) -- under a row partition the
// input needs one more ghost row each side than the output (the CA schedule's depths provide it).
constexpr int kRA = kMB + 4;   // ring A (x_in) and the thn ring: columns c0-2 .. c0+257
template <int W, int OFF>
struct XRingW {
    const double* x;   // [4][3][W]: tile column 0 is grid column c0 - OFF
    int s[3];
    int gr, c0;
    __device__ double X(int f, int r, int c) const { return x[(f * 3 + s[r - gr + 1]) * W + (c - c0 + OFF)]; }
};
struct Fused2 {
    const double* x_in;
    const double* d_in;
    const double* b;      // BNone: the right-hand side; GxB: unused (recomputed from x_p)
    const double* sub;    // SUB: the solve's last sweep returns sub - x
    double* x_out;
    double* d_out;        // SD: level B's direction is stored
    double c1a, c2a, c1b, c2b;
};
struct Stage2 {
    double x[4], xh[4];   // x_in at the lane's column c0-2+tid and (lanes 0..3) c0+254+tid
    double t, th;         // thn at the same columns
};
template <class BS>
struct OpsA {             // level A's operands at one column of row t
    double d[4], face[2];
    typename BS::Q q;
    double b[4];
};

template <bool SUB, bool SD, class BS>
__global__ void __launch_bounds__(kMB) __attribute__((amdgpu_waves_per_eu(2, 8)))
k_march2(FStencilFast P, Fused2 a, int nchunks, BS bs) {
    __shared__ double ra[4 * 3 * kRA];
    __shared__ double rb[4 * 3 * kMTileW];
    __shared__ double st[5 * kRA];
    const int n = P.n;
    const int strips = (n + kMB - 1) / kMB;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int strip = bk % strips, chunk = bk / strips;
    int la, lb;
    if (!march_rows(P.which, P.L, P.ext, chunk, nchunks, &la, &lb)) return;
    const int c0 = strip * kMB, tid = threadIdx.x;
    const int cm = c0 - 2 + tid, ch = c0 + kMB - 2 + tid;   // staged columns (ch: lanes 0..3)
    const bool okm = cm <= n + 1, okh = tid < 4 && ch <= n + 1;
    const int gm = okm ? P.wrap(cm) : 0, gh = okh ? P.wrap(ch) : gm;
    const int gc = c0 + tid;                                  // levels A and B: the lane's column
    const bool liveA = gc <= n, liveB = gc < n;
    const int gcl = liveB ? gc : 0;                           // operand column (column n: level A's halo, wraps to 0)
    const int gca = liveA ? P.wrap(gc) : 0;
    // lanes 0, 1: level A's halo columns c0-1, c0+256 (extra pass)
    const int cx = tid == 0 ? c0 - 1 : c0 + kMB;
    const bool liveX = tid < 2 && cx <= n;
    const int gcx = liveX ? P.wrap(cx) : gca;
    auto xslot = [&](int r) { return (r - la + 2) % 3; };   // ring A (rows >= la-2)
    auto tslot = [&](int r) { return (r - la + 2) % 5; };   // thn ring
    auto bslot = [&](int r) { return (r - la + 1) % 3; };   // ring B (rows >= la-1)
    auto grow = [&](int lr) { return P.wrap(P.r0 + lr); };
    // a row of the output layout: one GPU wraps level A's rows -1 and n periodically; a partition's ghost rows are in
    // the ext layout
    auto orow = [&](int lr) { return P.h == 0 ? P.wrap(lr) : lr; };
    auto load_stage = [&](int lr, Stage2& g) {
        const int gr = P.r0 + lr;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int32_t base = P.xrow(f, gr);
            g.x[f] = a.x_in[base + gm];
            g.xh[f] = a.x_in[base + gh];
        }
        const int32_t tb = P.wrap(gr) * n;
        g.t = P.cell[tb + gm];
        g.th = P.cell[tb + gh];
    };
    auto store_stage = [&](int lr, const Stage2& g) {
        const int xs = xslot(lr), ts = tslot(lr);
#pragma unroll
        for (int f = 0; f < 4; ++f) ra[(f * 3 + xs) * kRA + tid] = okm ? g.x[f] : 0.0;
        st[ts * kRA + tid] = okm ? g.t : 0.0;
        if (tid < 4) {
#pragma unroll
            for (int f = 0; f < 4; ++f) ra[(f * 3 + xs) * kRA + kMB + tid] = okh ? g.xh[f] : 0.0;
            st[ts * kRA + kMB + tid] = okh ? g.th : 0.0;
        }
    };
    // level A's operands at (local row lr, wrapped column g): d_in, the faces, b (or G x_p's operands)
    auto load_ops = [&](int lr, int g, OpsA<BS>& o) {
#pragma unroll
        for (int f = 0; f < 4; ++f) o.d[f] = a.d_in[P.out_row(f, orow(lr), g)];
        const int32_t k = grow(lr) * n + g;
        o.face[0] = P.uface[k];
        o.face[1] = P.vface[k];
        if constexpr (BS::on) o.q = bs.load(lr, grow(lr), g);
        else {
#pragma unroll
            for (int f = 0; f < 4; ++f) o.b[f] = a.b[P.out_row(f, orow(lr), g)];
        }
    };
    // level A at row lr, column c (virtual: -1 and n wrap): x_s into ring B, d_s and b returned
    auto level_a = [&](int lr, int c, const OpsA<BS>& o, double* dA, double* bA) {
        const int gr = grow(lr);
        const XRingW<kRA, 2> xa{ra, {xslot(lr - 1), xslot(lr), xslot(lr + 1)}, gr, c0};
        const TRingT<kRA, 2> ta{st, {tslot(lr - 1), tslot(lr), tslot(lr + 1)}, gr, c0};
        const FStencilDev::Cell cl{{o.face[0], o.face[1]}};
        double acc[4], rd[4];
        P.rows4(gr, c, ta, xa, cl, acc, rd);
        const int bsl = bslot(lr);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            double bf;
            if constexpr (BS::on) bf = bs.b(f, gr, c, P.wrap(c), ta, o.q);
            else bf = o.b[f];
            const double z = (bf - acc[f]) * rd[f];
            const double dn = a.c1a * o.d[f] + a.c2a * z;
            rb[(f * 3 + bsl) * kMTileW + (c - c0 + 1)] = xa.X(f, gr, c) + dn;
            dA[f] = dn;
            bA[f] = bf;
        }
    };
    // prologue: x_in and thn rows la-2, la-1 in the rings, row la in registers
    Stage2 g;
    {
        Stage2 g0, g1;
        load_stage(la - 2, g0);
        load_stage(la - 1, g1);
        load_stage(la, g);
        store_stage(la - 2, g0);
        store_stage(la - 1, g1);
    }
    double dP[4] = {0.0, 0.0, 0.0, 0.0}, bP[4] = {0.0, 0.0, 0.0, 0.0}, fP[2] = {0.0, 0.0};   // level A of row t-1
    auto step = [&](int t, auto load_next) {
        store_stage(t + 1, g);
        OpsA<BS> oa, ox;
        load_ops(t, gca, oa);
        load_ops(t, gcx, ox);
        double sv[4] = {0.0, 0.0, 0.0, 0.0};
        const bool doB = t - 1 >= la;
        if constexpr (SUB) {
#pragma unroll
            for (int f = 0; f < 4; ++f) sv[f] = a.sub[P.out_row(f, orow(t - 1), gcl)];
        }
        __syncthreads();
        if constexpr (decltype(load_next)::value) load_stage(t + 2, g);
        double dA[4] = {0.0, 0.0, 0.0, 0.0}, bA[4] = {0.0, 0.0, 0.0, 0.0};
        if (liveA) level_a(t, gc, oa, dA, bA);
        if (liveX) {
            double dx[4], bx[4];
            level_a(t, cx, ox, dx, bx);
        }
        __syncthreads();
        if (doB && liveB) {   // level B: row t-1 from ring B
            const int lr = t - 1, gr = grow(lr);
            const XRingW<kMTileW, 1> xa{rb, {bslot(lr - 1), bslot(lr), bslot(lr + 1)}, gr, c0};
            const TRingT<kRA, 2> ta{st, {tslot(lr - 1), tslot(lr), tslot(lr + 1)}, gr, c0};
            const FStencilDev::Cell cl{{fP[0], fP[1]}};
            double acc[4], rd[4];
            P.rows4(gr, gc, ta, xa, cl, acc, rd);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double z = (bP[f] - acc[f]) * rd[f];
                const double dn = a.c1b * dP[f] + a.c2b * z;
                const int32_t o = P.out_row(f, orow(lr), gc);
                if constexpr (SD) a.d_out[o] = dn;
                const double x = xa.X(f, gr, gc) + dn;
                a.x_out[o] = SUB ? sv[f] - x : x;
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            dP[f] = dA[f];
            bP[f] = bA[f];
        }
        fP[0] = oa.face[0];
        fP[1] = oa.face[1];
    };
    for (int t = la - 1; t < lb; ++t) step(t, std::true_type{});
    step(lb, std::false_type{});
}

// Workgroups of one marching-kernel instance the device holds at once (occupancy x CUs), queried once.
template <auto K>
int64_t march_capacity() {
    static int64_t cap = -1;
    if (cap < 0) {
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, K, kMB, 0) != hipSuccess)
            cus = per_cu = 0;
        cap = (int64_t)cus * per_cu;
    }
    return cap;
}

// Launch k_march over the partition rows P.which selects, rows_per_block rows per workgroup -- except that
// a launch up to 25 % over one round of workgroups is rebalanced into exactly one round (chunks of
// rows_per_block or rows_per_block + 1 rows): a second round of a few workgroups would cost almost a whole
// sweep's latency (ghost-row launches of the CA schedule, multi-GPU row partitions).
// Chunks (workgroup row ranges) of a marching launch over the rows P.which selects; 0: nothing to do.
template <class S>
int64_t march_chunks(const S& P, int rows_per_block, int64_t capacity) {
    const int64_t grows = P.which == 0 ? P.L : P.which == 1 ? (P.L > 2 ? P.L - 2 : 0)
                          : P.which == 3 ? P.L + 2 * P.ext : (P.L >= 2 ? 2 : 1);
    if (grows == 0) return 0;
    const int64_t strips = (P.n + kMB - 1) / kMB;
    if (rows_per_block <= 0) {   // auto: the rows per workgroup that fill one round (1024^2: 4; 2048^2: 16; 512^2: 1)
        const int64_t fill = capacity > 0 ? grows * strips / capacity : 4;
        rows_per_block = (int)(fill < 1 ? 1 : fill > 16 ? 16 : fill);
    }
    int64_t chunks = P.which == 2 ? grows : (grows + rows_per_block - 1) / rows_per_block;
    if (P.which != 2) {
        const int64_t one_round = capacity / strips;
        if (one_round > 0 && chunks > one_round && chunks * 4 <= one_round * 5) chunks = one_round;
    }
    return chunks;
}

template <class S, class XS, class Epi, class BS = BNone>
int launch_march_fixed(const S& P, const XS& xs, Epi epi, int rows_per_block, hipStream_t st, const BS& bs = BS{}) {
    // D, G, Gt_G on one GPU, and (KO().f_direct) the tolerance-mode F rows: the direct kernel
    if constexpr ((!std::is_base_of_v<FStencilDev, S> && !BS::on) || S::kFast) {
        if (S::kFast ? KO().f_direct != 0 : KO().pg_direct != 0) {
            // rows as march_rows: 0 all owned, 1 rows 1 .. L-2, 2 rows 0 and L-1, 3 owned + ext ghost rows each side
            const int la = P.which == 1 ? 1 : P.which == 3 ? -P.ext : 0;
            const int lb = P.which == 1 ? P.L - 1 : P.which == 3 ? P.L + P.ext : P.L;
            const int rows = P.which == 2 ? (P.L >= 2 ? 2 : 1) : lb - la;
            if (rows <= 0) return MPBP_OK;
            const int64_t cells = (int64_t)rows * P.n;
            k_direct<S, XS, Epi, BS><<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(P, xs, epi, la, rows, bs);
            MPBP_HIP(hipGetLastError());
            return MPBP_OK;
        }
    }
    const int64_t chunks = march_chunks(P, rows_per_block, march_capacity<k_march<S, XS, Epi, BS>>());
    if (chunks == 0) return MPBP_OK;
    const int64_t strips = (P.n + kMB - 1) / kMB;
    k_march<S, XS, Epi, BS><<<(unsigned)(chunks * strips), kMB, 0, st>>>(P, xs, (int)chunks, epi, bs);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

}  // namespace

#include "f_tile.inc"
#include "f_solve_w.inc"
#include "pg_stencil.inc"
#include "gtg_solve.inc"
#include "mg_fused.inc"
#include "launchers.inc"
#include "abi_core.inc"
#include "krylov.inc"
#include "abi_stencil.inc"
#include "q13.inc"
#include "schur_ops.inc"
#include "mg_coupled.inc"
#include "mg_solve.inc"
#include "mg_accel.inc"
#include "schur_inner.inc"
#include "schur_apply.inc"
#include "abi_mg.inc"

// Placement pad.  The code object's .text follows its metadata and .rodata, so adding kernels moves every kernel's
// offset within its 4 KB page.  With the partitioned A instances added, .text went from page offset 0x800 to 0x900
// and bench.py's apply -- byte-identical kernels -- measured 0.9-1.0 % slower in alternating runs (6980-7006 against
// 7059-7068 applies/s); these 0xF00 read-only bytes put .text back at 0x800 (7045-7078).  DESIGN.md section 4f.
// Re-derive or drop it when the kernel set changes (llvm-objdump -h on the unbundled gfx950 code object).
// Re-derived with the any-size transfer and wide product kernels: their descriptors and metadata moved .text by
// 0x3900 (to page offset 0x100 under the 0xF00 pad); 0x600 puts it back at 0x800.
extern "C" __device__ __attribute__((used)) const char mpbp_text_pad[0x600] = {1};
