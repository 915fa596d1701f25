"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the any-size coarsening rule (mg.Multigrid(coarsen="any"),
mpbp_mg_transfer_any_*), shared by tests/test_mg_any_restatement.py (CPU) and tests/test_gpu_mg_any.py.

Only the 1D interpolation and the stopping rule differ from oracle/mg_oracle.py: fine size nf >= 5 coarsens to
nc = nf // 2, each fine point is interpolated linearly from its two coarse neighbours on the periodic grid, the weights
one IEEE division of two exact integers each (include/mpbp.h).  The Kronecker products, R = P^T, the Galerkin products
(csr_oracle.spgemm) and the cycle are the oracle's own.
"""
import numpy as np
import scipy.sparse as sp

from oracle import csr_oracle as co
from oracle import mg_oracle as mo

CELL, NODE = mo.CELL, mo.NODE


def p1d_lists(nf: int, kind: int):
    """Per fine index f, the sorted list [(coarse index, weight)] of the rule, from integers only."""
    assert nf >= 5
    nc = nf // 2
    rows = []
    for f in range(nf):
        if kind == NODE:
            num, den = f * nc, nf
        else:
            num, den = (2 * f + 1) * nc - nf, 2 * nf   # negative at f = 0: Python's // floors towards -inf
        i0 = num // den
        rem = num - i0 * den
        if rem == 0:
            row = [(i0 % nc, 1.0)]
        else:
            row = [(i0 % nc, np.float64(den - rem) / np.float64(den)), ((i0 + 1) % nc, np.float64(rem) / np.float64(den))]
        rows.append(sorted(row))
    return rows


def p1d(nf: int, kind: int) -> sp.csr_matrix:
    """1D interpolation fine nf -> coarse nf // 2 as CSR (sorted indices)."""
    rows = p1d_lists(nf, kind)
    indptr = np.cumsum([0] + [len(r) for r in rows])
    M = sp.csr_matrix((np.array([w for r in rows for _, w in r], dtype=np.float64),
                       np.array([i for r in rows for i, _ in r], dtype=np.int32), indptr), shape=(nf, nf // 2))
    M.sort_indices()
    return M


def transfer(n: int, fields, which: str) -> sp.csr_matrix:
    """mg_oracle.transfer with the general p1d."""
    P = sp.block_diag([sp.kron(p1d(n, ky), p1d(n, kx)) for ky, kx in fields], format="csr")
    P.eliminate_zeros()
    M = sp.csr_matrix(P if which == "P" else P.T.tocsr())
    M.sort_indices()
    return M


def stop(m: int, coarsest: int, nlevels: int) -> bool:
    return (m <= coarsest and nlevels > 1) or m < 5


def level_sizes(n: int, coarsest: int):
    sizes = [n]
    while not stop(sizes[-1], coarsest, len(sizes)):
        sizes.append(sizes[-1] // 2)
    return sizes


def hierarchy(A, n, fields, coarsest=8, keep_inner=None):
    """[(A_l, n_l)], [P_l], [R_l] with floor halving; keep_inner (a list) receives the A P intermediates."""
    ops, Ps, Rs = [(sp.csr_matrix(A), n)], [], []
    m = n
    while not stop(m, coarsest, len(ops)):
        P, R = transfer(m, fields, "P"), transfer(m, fields, "R")
        AP = co.spgemm(A, P)
        if keep_inner is not None:
            keep_inner.append(AP)
        A = co.spgemm(R, AP)
        Ps.append(P)
        Rs.append(R)
        m //= 2
        ops.append((A, m))
    return ops, Ps, Rs


class MgAnyOracle(mo.MgOracle):
    """oracle.mg_oracle.MgOracle over the any-size hierarchy (the cycle is inherited unchanged)."""

    def __init__(self, A, n, fields, pre=2, post=2, cycles=1, ratio=4.0, coarsest=8, bounds=None, coarse_inv=None):
        self.ops, self.P, self.R = hierarchy(A, n, fields, coarsest)
        self.diags = [np.asarray(M.diagonal(), dtype=np.float64) for M, _ in self.ops]
        if bounds is None:
            bounds = []
            for (M, _), d in zip(self.ops, self.diags):
                lmax = mo.gershgorin(M, d)
                bounds.append((lmax / ratio, lmax))
        self.bounds = bounds
        self.pre, self.post, self.cycles = pre, post, cycles
        Ac = self.ops[-1][0].toarray()
        self.coarse_inv = np.linalg.pinv(Ac, rcond=mo.COARSE_RCOND) if coarse_inv is None else np.asarray(coarse_inv)
        m = self.coarse_inv.shape[0]
        self._cinv = sp.csr_matrix((self.coarse_inv.reshape(-1), np.tile(np.arange(m), m),
                                    np.arange(0, m * m + 1, m)), shape=(m, m))


def contraction(ora, A, steps=8, seed=0, project_mean=False):
    """Multigrid.contraction's power iteration on E = I - M A with the oracle's cycle; project_mean: the constant mode
    (Gt_G's null space) taken out of every iterate."""
    e = np.random.default_rng(seed).standard_normal(A.shape[0])
    if project_mean:
        e = e - e.mean()
    norm = float(np.linalg.norm(e))
    ratios = []
    for _ in range(steps):
        e = e - ora.solve(co.spmv(A, e))
        if project_mean:
            e = e - e.mean()
        new = float(np.linalg.norm(e))
        ratios.append(new / norm)
        norm = new
    return ratios
