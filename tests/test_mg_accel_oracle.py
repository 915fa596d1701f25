"""CPU checks of the Chebyshev acceleration of multigrid V-cycles (InnerSolver("mg", K, accel="chebyshev")): the numpy
restatement of the recurrence (tests/mg_accel_restatement.py) against the Chebyshev polynomials' closed form, its effect
over oracle/mg_oracle.py's V-cycle, and the argument checks that need no GPU."""
import numpy as np
import pytest

import mg_accel_restatement as ar


@pytest.fixture(scope="module")
def mo(oracle_built):
    from oracle import mg_oracle
    return mg_oracle


def _cheb_T(K, x):
    """T_K(x) in closed form: cos(K arccos x) on [-1, 1] (an endpoint that rounding put an ulp outside is the
    endpoint), cosh(K arccosh x) above."""
    x = np.asarray(x, dtype=np.float64)
    inside = np.abs(x) <= 1.0 + 1e-14
    out = np.empty_like(x)
    out[inside] = np.cos(K * np.arccos(np.clip(x[inside], -1.0, 1.0)))
    out[~inside] = np.cosh(K * np.arccosh(x[~inside]))
    return out


@pytest.mark.parametrize("rho", [0.05, 0.1, 0.375])
@pytest.mark.parametrize("K", range(1, 9))
def test_recurrence_is_the_chebyshev_polynomial(K, rho):
    """M = I, A = diag(lambda) with lambda on a grid in [1 - rho, 1]: one 'cycle' from x is x + (b - lambda x), and the
    error of x_K is T_K((theta - lambda) / delta) / T_K(theta / delta) -- the closed form, not a copy of the recurrence."""
    lam = np.linspace(1.0 - rho, 1.0, 41)
    b = lam.copy()                               # exact solution: ones
    vcycle = lambda b_, x: b_.copy() if x is None else x + (b_ - lam * x)
    x = ar.accel_solve(vcycle, b, K, rho)
    theta, delta = 1.0 - rho / 2.0, rho / 2.0
    want = _cheb_T(K, (theta - lam) / delta) / _cheb_T(K, np.array([theta / delta]))[0]
    assert np.max(np.abs((1.0 - x) - want)) <= 1e-13
    # sub: the last step's out = sub - x, the same x
    sub = np.linspace(-1.0, 2.0, lam.size)
    assert np.array_equal(ar.accel_solve(vcycle, b, K, rho, sub=sub), sub - x)


@pytest.mark.parametrize("n,coarsest", [(16, 8), (32, 16)])
def test_accelerated_residual_below_stationary(mo, n, coarsest):
    """F at eta_n = 100, V(2,2): with rho from the estimator, K accelerated cycles leave a strictly smaller residual
    than K stationary ones for K = 2, 3, 4, 6."""
    from oracle.stokes_oracle import StokesSystem
    S = StokesSystem(n, 1.0, 100.0, 1.0)
    ora = mo.MgOracle(S.F, n, mo.FIELDS_VELOCITY, coarsest=coarsest)
    vcycle = ar.oracle_vcycle(ora)
    ratios, _ = ar.contraction(S.F, vcycle)
    rho = ar.estimate_rho(ratios)
    assert 0.0 < rho < 0.5, (ratios, rho)
    b = np.random.default_rng(n).standard_normal(S.F.shape[0])
    nb = np.linalg.norm(b)
    for K in (2, 3, 4, 6):
        res_s = np.linalg.norm(b - S.F @ ar.stationary_solve(vcycle, b, K)) / nb
        res_a = np.linalg.norm(b - S.F @ ar.accel_solve(vcycle, b, K, rho)) / nb
        print(f"n={n} K={K} rho={rho:.4f}: stationary {res_s:.3e}, accelerated {res_a:.3e}")
        assert res_a < res_s, (K, res_a, res_s)


def test_stationary_restatement_is_the_oracle_solve(mo):
    """K plain cycles through the restatement's vcycle wrapper are MgOracle.solve's, bit for bit."""
    from oracle.stokes_oracle import StokesSystem
    S = StokesSystem(16, 1.0, 100.0, 1.0)
    ora = mo.MgOracle(S.F, 16, mo.FIELDS_VELOCITY, cycles=3)
    b = np.random.default_rng(3).standard_normal(S.F.shape[0])
    assert np.array_equal(ar.stationary_solve(ar.oracle_vcycle(ora), b, 3), ora.solve(b))


def test_inner_solver_argument_checks():
    import mp_block_preconditioners_amd as mp
    ok = mp.InnerSolver("mg", 3, accel="chebyshev", rho=0.1)
    assert (ok.accel, ok.rho) == ("chebyshev", 0.1)
    assert mp.InnerSolver("mg", 3).accel is None and mp.InnerSolver("mg", 3).rho is None
    with pytest.raises(ValueError, match="pre == post"):
        mp.InnerSolver("mg", 2, pre=1, post=3, accel="chebyshev")
    with pytest.raises(ValueError, match="accel"):
        mp.InnerSolver("mg", 2, accel="cg")
    with pytest.raises(ValueError, match="'mg'"):
        mp.InnerSolver("chebyshev", 4, accel="chebyshev")
    with pytest.raises(ValueError, match="'mg'"):
        mp.InnerSolver("jacobi", 3, accel="chebyshev")
    with pytest.raises(ValueError, match="rho"):
        mp.InnerSolver("mg", 2, accel="chebyshev", rho=1.5)
    # the checks run again when the solver is resolved (fields of a dataclass can be set after construction)
    late = mp.InnerSolver("chebyshev", 4)
    late.accel = "chebyshev"
    with pytest.raises(ValueError, match="'mg'"):
        late.resolve(None, None)


def test_multigrid_argument_checks():
    """Multigrid refuses before it touches the operator (no GPU needed)."""
    import mp_block_preconditioners_amd as mp
    with pytest.raises(ValueError, match="pre == post"):
        mp.Multigrid(None, 16, mp.FIELDS_VELOCITY, pre=1, post=3, accel="chebyshev")
    with pytest.raises(ValueError, match="accel"):
        mp.Multigrid(None, 16, mp.FIELDS_VELOCITY, accel="cg")


def test_distributed_constructor_refuses_acceleration():
    """Raised before any torch.distributed call: no process group is initialised here."""
    import torch.distributed as dist
    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd.distributed import DistributedSchurPreconditioner
    assert not (dist.is_available() and dist.is_initialized())
    for kw in (dict(inner_F=mp.InnerSolver("mg", 3, accel="chebyshev", rho=0.1)),
               dict(inner_P=mp.InnerSolver("mg", 3, accel="chebyshev", rho=0.1))):
        with pytest.raises(ValueError, match="row-partitioned"):
            DistributedSchurPreconditioner(16, 1.0, 100.0, 1.0, **kw)


@pytest.mark.parametrize("arg", ["halo", "f_mode", "pg_mode", "ca", "layout", "numerics"])
def test_distributed_constructor_checks_arguments_first(arg):
    """Every refusal that depends on an argument alone is raised before any torch.distributed call (no process group
    is initialised here; torch's own ValueError for that never reads "<argument> must be"): a bad argument on one rank
    cannot leave the others waiting in a collective."""
    import torch.distributed as dist
    from mp_block_preconditioners_amd.distributed import DistributedSchurPreconditioner
    assert not (dist.is_available() and dist.is_initialized())
    with pytest.raises(ValueError, match=rf"^{arg} must be"):
        DistributedSchurPreconditioner(16, 1.0, 100.0, 1.0, **{arg: "x"})


def test_distributed_operators_check_halo_first():
    """DistributedMatrix and DistributedStokesOperator refuse an unknown halo before any torch.distributed call."""
    import torch.distributed as dist
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.distributed import DistributedMatrix, DistributedStokesOperator
    from mp_block_preconditioners_amd.preconditioner import StokesOperator
    assert not (dist.is_available() and dist.is_initialized())
    with pytest.raises(ValueError, match=r"^halo must be"):
        DistributedMatrix(None, 16, 5, halo="x")
    prm = _lib.StokesParams()
    prm.n = 16
    with pytest.raises(ValueError, match=r"^halo must be"):
        DistributedStokesOperator(StokesOperator(prm, (None, None, None)), halo="x")
