"""CPU checks of tests/coupled_smoother_restatement.py, the restatement the GPU's phase-coupled smoother is compared with
bit for bit: its tables against dense 2 x 2 inverses, its bound against the dense spectral radius, and the conditions
the smoother exists for -- at drag xi = 1e6 the coupled V-cycle contracts and the point one does not; at xi = 1 they
agree."""
import functools

import numpy as np
import pytest

import coupled_smoother_restatement as cr
from oracle import mg_oracle as mo


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_built):
    return True


@functools.lru_cache(maxsize=None)
def _F(n, xi, eta_n, eta_s):
    from oracle.stokes_oracle import StokesSystem, theta_tables
    return StokesSystem(n, xi, eta_n, eta_s, 1.0, -1.0, tables=theta_tables(n)).F


PRMS = [(1.0, 100.0, 1.0), (1.0e6, 1.0, 1.0), (1.0e4, 1.0, 1.0e-4)]


@pytest.mark.parametrize("prm", PRMS)
@pytest.mark.parametrize("n", [8, 16])
def test_tables_are_the_dense_block_inverses(n, prm):
    """On F and every smoothed Galerkin level: [p_i, q_i] against row i's line of inv([[a, k], [k', a']]) computed in
    exact rational arithmetic from the stored doubles (so the reference has no error of its own).

    The bar.  With u = 2^-53, the stated order det = fl(fl(a a') - fl(k k')) has |det_fl - det| <= u (|a a'| + |k k'|)
    + u |det| to first order, and the division adds u: the relative error of p and q is at most u (kappa + 2) with
    kappa = (|a a'| + |k k'|) / det, asserted as u (kappa + 3) (one u for the second-order terms).  That is below the
    1e-14 the tables are specified to whenever kappa <= 87, which holds at xi = 1 (asserted).  At xi = 1e6 the block is
    [[xi t + ., -xi t], [-xi t, xi t + .]] with kappa ~ 2 xi t h^2 / eta (measured: up to 1.95e3 at n = 8, 488 at
    n = 16): a a' - k k' cancels, the stated operation order cannot reach 1e-14 there (measured errors up to 1.1e-13 at
    n = 8, 3.7e-14 at n = 16, against bars of 2.2e-13 and 5.5e-14), and the bar is the format's."""
    from fractions import Fraction
    u = 2.0 ** -53
    ora = cr.CoupledMgOracle(_F(n, *prm), n)
    assert len(ora.cpl) == len(ora.ops) - 1 >= 1
    worst = kmax = 0.0
    for (M, _), (p, q) in zip(ora.ops, ora.cpl):
        N = M.shape[0]
        pi = cr.partner(N)
        Md = M.toarray()
        for i in range(N):
            a, k, k2, a2 = (Fraction(float(Md[r, c])) for r, c in ((i, i), (i, pi[i]), (pi[i], i), (pi[i], pi[i])))
            det = a * a2 - k * k2
            assert det > 0
            kappa = float((abs(a * a2) + abs(k * k2)) / det)
            for got, want in ((p[i], a2 / det), (q[i], -k / det)):
                err = float(abs(Fraction(float(got)) - want) / abs(want)) if want else abs(float(got))
                assert err <= u * (kappa + 3.0), (i, err, kappa)
                worst = max(worst, err)
            kmax = max(kmax, kappa)
    print(f"coupled tables n={n} prm={prm}: worst relative error {worst:.2e}, largest kappa {kmax:.3g}")
    if prm[0] == 1.0:
        assert kmax <= 87.0 and worst <= 1e-14, (kmax, worst)


@pytest.mark.parametrize("prm", PRMS)
def test_bound_dominates_the_dense_spectral_radius(prm):
    """n = 8: lmax = ||B^-1 A||_inf >= rho(B^-1 A) on every smoothed level, and the vectorised bound is the literal
    two-pointer merge's, bit for bit."""
    n = 8
    ora = cr.CoupledMgOracle(_F(n, *prm), n)
    for (M, _), (p, q), (lmin, lmax) in zip(ora.ops, ora.cpl, ora.bounds):
        N = M.shape[0]
        pi = cr.partner(N)
        Md = M.toarray()
        Binv = np.zeros((N, N))
        Binv[np.arange(N), np.arange(N)] = p
        Binv[np.arange(N), pi] = q
        rho = float(np.max(np.abs(np.linalg.eigvals(Binv @ Md))))
        assert lmax >= rho * (1.0 - 1e-12), (lmax, rho)
        assert lmax == cr.bound_literal(M, p, q) and lmin == lmax / 4.0
        print(f"coupled bound n={n} prm={prm} rows={N}: lmax {lmax:.4f}, spectral radius {rho:.4f}")


def test_bad_blocks_name_the_row():
    import scipy.sparse as sp
    F = sp.csr_matrix(_F(8, 1.0, 100.0, 1.0), copy=True)
    F.sort_indices()
    e = F.indptr[5] + int(np.flatnonzero(F.indices[F.indptr[5]:F.indptr[6]] == 5)[0])
    F.data[e] = 0.0   # a stored zero diagonal: det = -k k' <= 0
    with pytest.raises(ValueError, match="row 5"):
        cr.tables(F)


def _point_contraction(F, n, steps):
    import mg_accel_restatement as ar
    ora = mo.MgOracle(F, n, mo.FIELDS_VELOCITY)
    return ar.contraction(F, ar.oracle_vcycle(ora), steps=steps)[0]


def test_coupled_contracts_at_large_drag_where_point_does_not():
    """n = 32, eta 1 / 1, xi = 1e6, V(2,2), ratio 4, coarsest 8, 25 power steps: coupled < 0.3, point > 0.8 (a scipy
    study of the same cycle measured 0.104 and 0.974)."""
    n = 32
    F = _F(n, 1.0e6, 1.0, 1.0)
    coupled = cr.contraction(cr.CoupledMgOracle(F, n), F, steps=25)[-1]
    point = _point_contraction(F, n, 25)[-1]
    print(f"contraction n={n} xi=1e6 eta 1/1: coupled {coupled:.4f}, point {point:.4f}")
    assert coupled < 0.3 and point > 0.8, (coupled, point)


def test_coupled_equals_point_at_unit_drag():
    """xi = 1 (eta 100 / 1, n = 32): the two contractions agree within 5 % (the study: equal to three digits)."""
    n = 32
    F = _F(n, 1.0, 100.0, 1.0)
    coupled = cr.contraction(cr.CoupledMgOracle(F, n), F, steps=25)[-1]
    point = _point_contraction(F, n, 25)[-1]
    print(f"contraction n={n} xi=1 eta 100/1: coupled {coupled:.4f}, point {point:.4f}")
    assert abs(coupled - point) <= 0.05 * point, (coupled, point)
