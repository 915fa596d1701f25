"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the four block forms of the Schur preconditioner apply
(mpbp_schur_plan.form, ApproxSchurPreconditioner(form=...)), shared by tests/test_block_forms_restatement.py (CPU) and
tests/test_gpu_block_forms.py.  With P = Gt_G, Q = Gt_F_G, S~^-1 = P^-1 Q P^-1 and every ^-1 an inner solve from x0 = 0:

    full:     y = F^-1 v_u ; x_p = S~^-1 (D y + v_p) ; u = y - F^-1 (G x_p)     approx_schur_op, solve.py:257-277
    upper:    x_p = S~^-1 v_p ; u = F^-1 (v_u - G x_p)                          inverse of [[F, G], [0, S]]
    lower:    u = F^-1 v_u ; x_p = S~^-1 (D u + v_p)                            inverse of [[F, 0], [-D, S]]
    diagonal: u = F^-1 v_u ; x_p = S~^-1 v_p                                    inverse of [[F, 0], [0, S]]

each returning [u, x_p].  Every step is one of oracle/'s: schur_oracle.inner_solve (Jacobi, Chebyshev, exact),
csr_oracle.spmv (mode 1 for D u + v_p, mode 2 for v_u - G x_p), mg_oracle's V-cycles and mg_accel_restatement's
accelerated ones -- the operation order of the GPU kernels, so exact numerics are compared bit for bit."""
import numpy as np

import mg_accel_restatement as ar
from oracle import csr_oracle as co
from oracle import schur_oracle as so

FORMS = ("full", "upper", "lower", "diagonal")


def solver(M, diag, inner, dense_inv=None):
    """solve(b, sub=None) of an inner-solver description: a schur_oracle.Inner, or a callable taken as it is
    (mg_solver / mg_accel_solver below)."""
    if callable(inner):
        return inner
    return lambda b, sub=None: so.inner_solve(M, diag, inner, np.ascontiguousarray(b, dtype=np.float64), sub=sub,
                                              dense_inv=dense_inv)


def mg_solver(ora):
    """The oracle hierarchy's own `cycles` stationary V-cycles (oracle.mg_oracle.MgOracle.solve)."""
    return lambda b, sub=None: ora.solve(b, sub)


def mg_accel_solver(ora, K, rho):
    """K Chebyshev-accelerated V-cycles of the oracle hierarchy (mg_accel_restatement.accel_solve)."""
    vc = ar.oracle_vcycle(ora)
    return lambda b, sub=None: ar.accel_solve(vc, np.ascontiguousarray(b, dtype=np.float64), K, rho, sub=sub)


def apply(form, F, D, G, GtG, GtFG, v, inner_F, inner_P, diag_F=None, diag_P=None, F_inv=None, GtG_inv=None):
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}")
    nu = F.shape[0]
    diag_F = so.diagonal(F) if diag_F is None else diag_F
    diag_P = so.diagonal(GtG) if diag_P is None else diag_P
    solve_F = solver(F, diag_F, inner_F, F_inv)
    solve_P = solver(GtG, diag_P, inner_P, GtG_inv)
    v = np.ascontiguousarray(v, dtype=np.float64)
    v_u, v_p = np.ascontiguousarray(v[:nu]), np.ascontiguousarray(v[nu:])

    def schur(rhs):   # S~^-1 rhs = P^-1 Q P^-1 rhs                         solve.py:265-271
        x_a = solve_P(rhs)
        x_b = co.spmv(GtFG, x_a)
        return solve_P(x_b)

    if form == "upper":
        x_p = schur(v_p)
        u = solve_F(co.spmv(G, x_p, v_u, mode=2))
        return np.concatenate([u, x_p])
    y = solve_F(v_u)
    if form == "diagonal":
        return np.concatenate([y, schur(v_p)])
    x_p = schur(co.spmv(D, y, v_p, mode=1))
    if form == "lower":
        return np.concatenate([y, x_p])
    u = solve_F(co.spmv(G, x_p), sub=y)
    return np.concatenate([u, x_p])
