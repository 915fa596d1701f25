"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the Chebyshev acceleration of multigrid V-cycles
(mpbp_mg_accel_coeffs, mpbp_mg_combine, mg.Multigrid(accel="chebyshev")), shared by tests/test_mg_accel_oracle.py (CPU)
and tests/test_gpu_mg_accel.py.  Every floating-point operation is written out in the order include/mpbp.h states, so
the GPU results can be compared bit for bit; the cycle itself is oracle/mg_oracle.py's."""
import numpy as np

RHO_MARGIN = 1.1   # the product's ACCEL_RHO_MARGIN, restated


def accel_coeffs(rho, K):
    """(omega[K], mu[K]) for spec(M A) in [1 - rho, 1]."""
    theta = 1.0 - rho / 2.0
    delta = rho / 2.0
    r = delta / theta
    omega, mu = [1.0 / theta], [0.0]
    for _ in range(1, K):
        r_new = 1.0 / (2.0 * theta / delta - r)
        omega.append(2.0 * r_new / delta)
        mu.append(r_new * r)
        r = r_new
    return omega, mu


def combine(y, xk, xold, omega, mu, sub=None):
    """One step's combination; xk None: the k = 0 form x = omega y."""
    if xk is None:
        x = omega * y
    else:
        t1 = y - xk
        t2 = omega * t1
        t3 = xk + t2
        t4 = xk - xold
        t5 = mu * t4
        x = t3 + t5
    return x if sub is None else sub - x


def accel_solve(vcycle, b, K, rho, sub=None):
    """x_K of the accelerated iteration; vcycle(b, x) is one V-cycle from the guess x (None: from zero)."""
    omega, mu = accel_coeffs(rho, K)
    xk = xold = None
    for k in range(K):
        y = vcycle(b, xk)
        if xk is not None and xold is None:
            xold = np.zeros_like(xk)
        xk, xold = combine(y, xk, xold, omega[k], mu[k], sub if k == K - 1 else None), xk
    return xk


def stationary_solve(vcycle, b, K):
    x = None
    for _ in range(K):
        x = vcycle(b, x)
    return x


def oracle_vcycle(ora):
    """vcycle(b, x) of an oracle.mg_oracle.MgOracle."""
    return lambda b, x: ora.vcycle(0, np.ascontiguousarray(b, dtype=np.float64), x)


def contraction(A, vcycle, steps=8, seed=0, spmv=None):
    """Power iteration on E = I - M A: ||e_{j+1}|| / ||e_j|| with e_{j+1} = e_j - V(A e_j), e_0 seeded standard normal."""
    if spmv is None:
        from oracle import csr_oracle as co
        spmv = co.spmv
    e = np.random.default_rng(seed).standard_normal(A.shape[0])
    norm = float(np.linalg.norm(e))
    ratios, vectors = [], [e]
    for _ in range(steps):
        e = e - vcycle(spmv(A, e), None)
        new = float(np.linalg.norm(e))
        ratios.append(new / norm)
        norm = new
        vectors.append(e)
    return ratios, vectors


def estimate_rho(ratios):
    return RHO_MARGIN * max(ratios[-3:])
