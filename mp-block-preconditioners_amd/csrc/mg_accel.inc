// Chebyshev acceleration of the V-cycles (mg_accel_coeffs, k_mg_combine, mg_solve_accel) and mg_solve.  Continues
// schur_ops.inc's namespace; needs mpbp.hip's first section and mg_solve.inc (MgFine, mg_vcycle).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.
namespace {

// ---------------------------------------------------- Chebyshev acceleration of the V-cycles ----
// Coefficients of the semi-iteration over K cycles with spec(M A) in [1 - rho, 1] (mpbp_mg_accel_coeffs; host, double).
void mg_accel_coeffs(double rho, int K, double* omega, double* mu) {
    const double theta = 1.0 - rho / 2.0;
    const double delta = rho / 2.0;
    double r = delta / theta;
    omega[0] = 1.0 / theta;
    mu[0] = 0.0;
    for (int k = 1; k < K; ++k) {
        const double r_new = 1.0 / (2.0 * theta / delta - r);
        omega[k] = 2.0 * r_new / delta;
        mu[k] = r_new * r;
        r = r_new;
    }
}

// One step's combination, x = xk + omega (y - xk) + mu (xk - xold), out = x or sub - x, in mpbp_mg_combine's operation
// order (T: double or f64x2; the file is built without FMA contraction, so every operation rounds on its own).
// xk NULL: x = omega y (x_0 = x_{-1} = 0); xold NULL: x_{k-1} = 0 is not read (xk - 0 is xk, bit for bit).  The forms
// are told apart by the pointers, uniform over the grid: one kernel per access width instead of one per form.
template <class T>
__device__ inline T mg_combine_value(const T* y, const T* xk, const T* xold, const T* sub, double omega, double mu,
                                     int64_t i) {
    const T yv = y[i];
    T x;
    if (!xk) {
        x = omega * yv;
    } else {
        const T xv = xk[i];
        const T t1 = yv - xv;
        const T t2 = omega * t1;
        const T t3 = xv + t2;
        const T t4 = xold ? xv - xold[i] : xv;
        const T t5 = mu * t4;
        x = t3 + t5;
    }
    return sub ? sub[i] - x : x;
}
// A pure stream: up to four 8-byte reads and one write per element.  VEC: 16 bytes per lane (every pointer 16-byte
// aligned) and the odd last element by one lane; else one element per lane.  Grid-stride; the pointers carry no
// __restrict__: out may be xold (or any other operand), each lane reads its elements before it writes them.
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_mg_combine(int64_t n, const double* y, const double* xk, const double* xold,
                                                       double omega, double mu, const double* sub, double* out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const int64_t n2 = n >> 1;
        const f64x2 *y2 = reinterpret_cast<const f64x2*>(y), *xk2 = reinterpret_cast<const f64x2*>(xk),
                    *xo2 = reinterpret_cast<const f64x2*>(xold), *sub2 = reinterpret_cast<const f64x2*>(sub);
        f64x2* out2 = reinterpret_cast<f64x2*>(out);
        for (int64_t i = t0; i < n2; i += stride) out2[i] = mg_combine_value(y2, xk2, xo2, sub2, omega, mu, i);
        if ((n & 1) && t0 == 0) out[n - 1] = mg_combine_value(y, xk, xold, sub, omega, mu, n - 1);
    } else {
        for (int64_t i = t0; i < n; i += stride) out[i] = mg_combine_value(y, xk, xold, sub, omega, mu, i);
    }
}

constexpr int kCombineMaxBlocks = 2048;   // 8 workgroups per CU; longer vectors stride

int mg_combine(int64_t n, const double* y, const double* xk, const double* xold, double omega, double mu,
               const double* sub, double* out, hipStream_t st) {
    if (n < 0 || (n && (!y || !out)) || (!xk && xold))
        return set_error(MPBP_ERR_ARG, "mg_combine: needs y and out, and xk whenever xold is given");
    if (!n) return MPBP_OK;
    const uintptr_t bits = (uintptr_t)y | (uintptr_t)xk | (uintptr_t)xold | (uintptr_t)sub | (uintptr_t)out;
    const bool vec = (bits & 15) == 0;
    const int64_t units = vec ? (n + 1) / 2 : n;
    const unsigned grid = (unsigned)std::min<int64_t>((units + kBlock - 1) / kBlock, kCombineMaxBlocks);
    if (vec) k_mg_combine<true><<<grid, kBlock, 0, st>>>(n, y, xk, xold, omega, mu, sub, out);
    else k_mg_combine<false><<<grid, kBlock, 0, st>>>(n, y, xk, xold, omega, mu, sub, out);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// The accelerated form of mg_solve's loop: step k runs one V-cycle from x_k (step 0: the zero-start cycle, with its
// fused level-0 launches) and combines its result y_k with x_k and x_{k-1}.  x_k and x_{k-1} live in m->accel_x: the
// cycle ping-pongs between fine.x and fine.t and only reads an initial guess that is a third buffer (mg_smooth's
// `spare`), so both survive it; the combination overwrites x_{k-1} with x_{k+1} (the last one writes
// x_out, as sub - x when sub is set).
int mg_solve_accel(const mpbp_mg* m, const MgFine& fine, const double* b, double* x_out, const double* sub,
                   hipStream_t st) {
    const int K = m->cycles;
    if (m->accel != MPBP_MG_ACCEL_CHEBYSHEV) return set_error(MPBP_ERR_ARG, "mg: unknown acceleration %d", m->accel);
    if (m->part_levels > 0)
        return set_error(MPBP_ERR_ARG, "mg: Chebyshev acceleration is not available on a row-partitioned hierarchy "
                                       "(part_levels = %d): use accel = 0 there", m->part_levels);
    if (K > 64 || !(m->accel_rho > 0.0) || !(m->accel_rho < 1.0))
        return set_error(MPBP_ERR_ARG, "mg: acceleration needs cycles <= 64 and 0 < accel_rho < 1 (got %d, %g)", K,
                         m->accel_rho);
    double* X[2] = {m->accel_x[0], m->accel_x[1]};
    if (K > 1 && (!X[0] || !X[1] || X[0] == X[1]))
        return set_error(MPBP_ERR_ARG, "mg: acceleration needs two distinct accel_x vectors");
    for (int i = 0; i < 2 && K > 1; ++i)
        if (X[i] == fine.x || X[i] == fine.t || X[i] == fine.r || X[i] == fine.d || X[i] == x_out || X[i] == b ||
            X[i] == sub)
            return set_error(MPBP_ERR_ARG, "mg: accel_x must not alias the level-0 work buffers, b, sub or x_out");
    double omega[64], mu[64];
    mg_accel_coeffs(m->accel_rho, K, omega, mu);
    const int64_t n = m->levels[0].nrows;
    int xk = 0;   // X[xk] = x_k, X[1 - xk] = x_{k-1} (k >= 1)
    for (int k = 0; k < K; ++k) {
        const bool last = k == K - 1;
        double* y = nullptr;
        int rc = mg_vcycle(m, 0, fine, b, k == 0, k == 0 ? fine.x : X[xk], nullptr, nullptr, &y, st);
        if (rc) return rc;
        double* out = last ? x_out : X[k == 0 ? 0 : 1 - xk];
        rc = mg_combine(n, y, k >= 1 ? X[xk] : nullptr, k >= 2 ? X[1 - xk] : nullptr, omega[k], mu[k],
                        last ? sub : nullptr, out, st);
        if (rc) return rc;
        if (k > 0) xk = 1 - xk;
    }
    return MPBP_OK;
}

// x_out = mg^-1 b by mg->cycles V-cycles from x = 0 (sub - that when sub != NULL).
int mg_solve(const mpbp_mg* m, const MgFine& fine, const double* b, double* x_out, const double* sub, hipStream_t st) {
    if (!m || m->nlevels < 2 || !m->levels || m->cycles < 1 || !m->coarse_inv.row_ptr)
        return set_error(MPBP_ERR_ARG, "mg: hierarchy needs >= 2 levels, >= 1 cycle and the coarse inverse");
    if (x_out == fine.x || x_out == fine.t || x_out == fine.r || x_out == fine.d || b == x_out)
        return set_error(MPBP_ERR_ARG, "mg: x_out must not alias the level-0 work buffers or b");
    if (int rc = mg_check_smoother(m)) return rc;
    if (m->accel) return mg_solve_accel(m, fine, b, x_out, sub, st);
    double* cur = fine.x;
    for (int k = 0; k < m->cycles; ++k) {
        const bool last = k == m->cycles - 1;
        double* res = nullptr;
        const int rc = mg_vcycle(m, 0, fine, b, k == 0, cur, last ? x_out : nullptr, last ? sub : nullptr, &res, st);
        if (rc) return rc;
        cur = res;
    }
    return MPBP_OK;
}

}  // namespace
