"""k_fsolve_w (the whole F solve on 32 x 16 tiles) after its staging, addressing and level 0 were trimmed: the same bits.

The kernel stages thn and x_p by wave-uniform rows, indexes every owned cell from one wrapped (row, column) pair, takes a
ring cell's coordinates from its lane range, and reads level 0's node averages from the LDS table the later levels use.
None of that may move a bit, so the full preconditioner apply through it (first solve: plain right-hand side; second:
sub - x with G x_p recomputed inside) is compared with torch.equal against the two paths that were not touched:
k_ftile / the marching kernels (kernel option f_solve = 0) and the 64 x 8 k_fsolve (f_solve_tile = 0).

Sizes: 72 (4 updates) and 70 (3 updates) are the smallest grids launch_fsolve accepts -- a tile's staged window wraps
onto the tile itself most tightly there (at n = 70 the 4-update solve falls back to the per-pair launches and is compared
all the same); 73 = 2 * 32 + 9 and 81 = 5 * 16 + 1 leave a ragged last tile column and row (the guards of cells past
the grid, staged lanes beyond a row's width); 96 is a whole number of tiles.  Coefficients: the bench's (xi 1, eta_n
100, eta_s 1, c 1) and a general set (xi 0.7, eta_n 1e4, eta_s 3, c 1.3) where no cached per-cell factor is 1.

At n = 72 the apply is also held to north_star's 1e-12 relative inf-norm of oracle/schur_oracle.py's apply
(TOL_APPLY of test_gpu_fast.py)."""
import numpy as np
import pytest

from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_APPLY = 1e-12   # north_star: fp64 residuals within 1e-12 relative inf-norm

COEFFS = {"bench": (1.0, 100.0, 1.0, 1.0, -1.0),       # xi, eta_n, eta_s, c, d_u
          "general": (0.7, 1.0e4, 3.0, 1.3, -1.0)}
SIZES = [70, 72, 73, 81, 96]

_SYSTEMS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(oracle_built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    _SYSTEMS.clear()


def _oracle_system(n, coef):
    """The oracle's operators of the case, built once for both update counts."""
    if (n, coef) not in _SYSTEMS:
        from oracle.stokes_oracle import StokesSystem, theta_tables
        xi, eta_n, eta_s, c, d_u = COEFFS[coef]
        _SYSTEMS[n, coef] = StokesSystem(n, xi, eta_n, eta_s, c, d_u, tables=theta_tables(n))
    return _SYSTEMS[n, coef]


@pytest.mark.parametrize("kf", [3, 4])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("coef", list(COEFFS))
def test_fsolve_w_bits(coef, n, kf):
    import mp_block_preconditioners_amd as mp
    from oracle.stokes_oracle import theta_tables
    xi, eta_n, eta_s, c, d_u = COEFFS[coef]
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*theta_tables(n))
    _, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u)
    pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("chebyshev", kf),
                                      inner_P=mp.InnerSolver("chebyshev", 4), numerics="fast")
    ko = pc.kernel_opts
    assert (ko.f_solve, ko.f_solve_tile, ko.f_pair, ko.f_tile) == (1, 1, 1, 1)   # the default is the kernel under test
    assert pc.fuse_g and pc.f_stencil is not None
    vh = np.random.default_rng(100 * n + kf).standard_normal(pc.shape[0])
    v = torch.from_numpy(vh).cuda()
    got = pc.apply(v).clone()
    assert bool(torch.isfinite(got).all())
    for opts in (dict(f_solve=0), dict(f_solve=1, f_solve_tile=0)):
        pc.set_kernel_opts(**opts)
        ref = pc.apply(v).clone()
        assert torch.equal(got, ref), (opts, float((got - ref).abs().max()))
    pc.set_kernel_opts(f_solve=1, f_solve_tile=1)
    assert torch.equal(pc.apply(v), got)
    if n == 72:
        from oracle.schur_oracle import Inner, approx_schur_apply
        S = _oracle_system(n, coef)
        want = approx_schur_apply(S.F, S.D, S.G, S.GtG, S.GtFG, vh,
                                  Inner("chebyshev", kf, pc.inner_F.lmin, pc.inner_F.lmax),
                                  Inner("chebyshev", 4, pc.inner_P.lmin, pc.inner_P.lmax))
        err = rel_inf(got.cpu().numpy(), want)
        print(f"fsolve_w {coef} n={n} kf={kf}: vs oracle {err:.3e}")
        assert 0.0 < err <= TOL_APPLY, err   # (> 0: the fast rows really ran)
