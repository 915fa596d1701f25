"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the phase-coupled multigrid smoother (mg.Multigrid(smoother="coupled"),
mpbp_cpl_blocks / mpbp_cpl_bound / mpbp_cpl_update), shared by tests/test_coupled_smoother_restatement.py (CPU) and
tests/test_gpu_coupled_smoother.py.

A level has nrows = 4 m^2 rows and H = nrows / 2; row i's partner is pi(i) = i + H for i < H, else i - H (u_n and u_s at
the same face, v_n and v_s likewise).  The smoother is Chebyshev on B^-1 A with B the 2 x 2 blocks [[a, k], [k', a']] of
the pairs.  Every floating-point operation is written in the order include/mpbp.h states (numpy evaluates element by
element without fused multiply-add), the residual is csr_oracle.spmv's, the hierarchy and the rest of the cycle are
oracle.mg_oracle.MgOracle's (or mg_any_restatement.MgAnyOracle's), so exact numerics are compared bit for bit.
"""
import numpy as np
import scipy.sparse as sp

import mg_any_restatement as anyr
from oracle import csr_oracle as co
from oracle import mg_oracle as mo
from oracle.schur_oracle import cheb_coeffs


def partner(nrows: int) -> np.ndarray:
    H = nrows // 2
    return np.concatenate([np.arange(H, nrows), np.arange(H)])


def _sorted(A) -> sp.csr_matrix:
    A = sp.csr_matrix(A, copy=True)
    A.sort_indices()
    return A


def _entries(A: sp.csr_matrix, cols: np.ndarray):
    """(value, stored) of A[i, cols[i]] per row; an entry that is not stored reads as +0.0."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    hit = A.indices == cols[rows]
    val, stored = np.zeros(n), np.zeros(n, dtype=bool)
    val[rows[hit]] = A.data[hit]
    stored[rows[hit]] = True
    return val, stored


def tables(A):
    """(cpl_p, cpl_q): det = a a' - k k', p = a' / det, q = (-k) / det.  ValueError naming the first bad row."""
    A = _sorted(A)
    n = A.shape[0]
    assert n % 4 == 0
    pi = partner(n)
    a, has_diag = _entries(A, np.arange(n))
    k, _ = _entries(A, pi)
    a2, k2 = a[pi], k[pi]
    with np.errstate(all="ignore"):
        det = a * a2 - k * k2
        p = a2 / det
        q = (-k) / det
    bad = ~has_diag | ~has_diag[pi] | ~np.isfinite(det) | ~(det > 0.0)
    if bad.any():
        raise ValueError(f"row {int(np.flatnonzero(bad)[0])}: no stored diagonal or det not finite and positive")
    return p, q


def bound(A, p, q) -> float:
    """max_i sum_c |p_i A[i,c] + q_i A[pi(i),c]| over the union of the two rows' columns, ascending, from 0.0.
    Vectorised: p_i A[i,:] and q_i A[pi(i),:] are formed entry by entry (one multiplication each), scipy's sparse sum
    adds them where both are stored; where one is absent the literal form adds p (+0.0) or q (+0.0), which changes at
    most the sign of a zero, and the absolute value removes that (bound_literal is the loop, compared on the CPU)."""
    A = _sorted(A)
    n = A.shape[0]
    pi = partner(n)
    Ap = sp.csr_matrix(A[pi, :])
    Ap.sort_indices()
    Sp = sp.csr_matrix((A.data * np.repeat(p, np.diff(A.indptr)), A.indices, A.indptr), shape=A.shape)
    Sq = sp.csr_matrix((Ap.data * np.repeat(q, np.diff(Ap.indptr)), Ap.indices, Ap.indptr), shape=A.shape)
    S = sp.csr_matrix(Sp + Sq)
    S.sort_indices()
    S.data = np.abs(S.data)
    return float(np.max(co.spmv(S, np.ones(n))))   # sequential row sums from 0.0 in column order; |v| * 1.0 = |v|


def bound_literal(A, p, q) -> float:
    """bound() as the two-pointer merge, one row at a time."""
    A = _sorted(A)
    n = A.shape[0]
    pi = partner(n)
    rp, ci, va = A.indptr, A.indices, A.data
    best = 0.0
    for i in range(n):
        e, e1, f, f1 = rp[i], rp[i + 1], rp[pi[i]], rp[pi[i] + 1]
        s = np.float64(0.0)
        while e < e1 or f < f1:
            ce = ci[e] if e < e1 else np.iinfo(np.int64).max
            cf = ci[f] if f < f1 else np.iinfo(np.int64).max
            c = min(ce, cf)
            v = va[e] if ce == c else np.float64(0.0)
            w = va[f] if cf == c else np.float64(0.0)
            s = s + abs(p[i] * v + q[i] * w)
            e += ce == c
            f += cf == c
        best = max(best, float(s))
    return best


def update(p, q, r, x, c1, c2, d, sub=None, dzero=False, store_d=True):
    """mpbp_cpl_update: z = p r + q r[pi]; d = c1 d + c2 z; x = x + d (x None: the zero start, x = d = c2 z, r is b).
    d is updated in place when store_d.  Returns x, or sub - x."""
    pi = partner(r.shape[0])
    z = p * r + q * r[pi]
    if x is None:
        dn = c2 * z
        xn = dn
    else:
        dv = np.zeros_like(d) if dzero else d
        dn = c1 * dv + c2 * z
        xn = x + dn
    if store_d:
        d[:] = dn
    return xn if sub is None else sub - xn


def smooth(A, p, q, lmin, lmax, K, b, x=None, sub=None):
    """K coupled sweeps from x (None: from 0, the first sweep is the init form); sub - x on the last."""
    c1, c2 = cheb_coeffs(lmin, lmax, K)
    d = np.zeros(A.shape[0])
    s = 0
    if x is None:
        x = update(p, q, b, None, 0.0, c2[0], d, sub if K == 1 else None, store_d=K > 1)
        s = 1
    for k in range(s, K):
        r = co.spmv(A, x, b, mode=2)
        x = update(p, q, r, x, c1[k], c2[k], d, sub if k == K - 1 else None, dzero=(k == 0), store_d=k < K - 1)
    return x


class _Coupled:
    """The coupled tables, intervals and cycle over a hierarchy built by the base oracle class."""

    def _init_coupled(self, ratio):
        self.cpl = [tables(M) for M, _ in self.ops[:-1]]
        self.bounds = []
        for (M, _), (p, q) in zip(self.ops[:-1], self.cpl):
            lmax = bound(M, p, q)
            self.bounds.append((lmax / ratio, lmax))

    def vcycle(self, l, b, x=None, sub=None):
        A, _ = self.ops[l]
        p, q = self.cpl[l]
        lmin, lmax = self.bounds[l]
        x = smooth(A, p, q, lmin, lmax, self.pre, b, x)
        r = co.spmv(A, x, b, mode=2)
        bc = co.spmv(self.R[l], r)
        xc = co.spmv(self._cinv, bc) if l + 1 == len(self.ops) - 1 else self.vcycle(l + 1, bc)
        x = co.spmv(self.P[l], xc, x, mode=1)
        return smooth(A, p, q, lmin, lmax, self.post, b, x, sub)


class CoupledMgOracle(_Coupled, mo.MgOracle):
    def __init__(self, A, n, fields=mo.FIELDS_VELOCITY, pre=2, post=2, cycles=1, ratio=4.0, coarsest=8,
                 coarse_inv=None):
        mo.MgOracle.__init__(self, A, n, fields, pre, post, cycles, ratio, coarsest, bounds=[], coarse_inv=coarse_inv)
        self._init_coupled(ratio)


class CoupledMgAnyOracle(_Coupled, anyr.MgAnyOracle):
    def __init__(self, A, n, fields=mo.FIELDS_VELOCITY, pre=2, post=2, cycles=1, ratio=4.0, coarsest=8,
                 coarse_inv=None):
        anyr.MgAnyOracle.__init__(self, A, n, fields, pre, post, cycles, ratio, coarsest, bounds=[], coarse_inv=coarse_inv)
        self._init_coupled(ratio)


def contraction(ora, A, steps=25, seed=0):
    """Power iteration on E = I - M A of one zero-start V-cycle: ||e_{j+1}|| / ||e_j|| per step (Multigrid.contraction)."""
    e = np.random.default_rng(seed).standard_normal(A.shape[0])
    norm = float(np.linalg.norm(e))
    ratios = []
    for _ in range(steps):
        e = e - ora.vcycle(0, co.spmv(A, e))
        new = float(np.linalg.norm(e))
        ratios.append(new / norm)
        norm = new
    return ratios
