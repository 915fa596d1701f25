"""The matrix-free system matrix (StokesOperator, mpbp_stokes_apply): A = [[F, d_p G], [d_div D, 0]] applied in one
marching launch with every row recomputed from the thn tables.

Exact numerics must reproduce the assembled row's sequential sum bit for bit -- a velocity row is F's row sum with the
two G products added to the same accumulator, a pressure row D's eight products scaled by d_div -- so the yardstick is
the sequential oracle's A u (n <= 64) and the CSR kernel on the assembled A a second, independently pinned witness.
Fast numerics (the regrouped F rows) stay within the project's 1e-12 relative inf-norm of the oracle, with the pressure
rows bit-identical to the exact result.  Shapes: every cell on the periodic edge (n = 3, 4, 5), an odd size whose
march_rows = 8 chunks are 8, 8 and 1 rows (17), one 256-column strip short / full / a second strip of one column whose
halo wraps to column 0 (255, 256, 257), and two strips (300)."""
import functools

import numpy as np
import pytest

from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_FAST = 1e-12   # the project's bar for fast numerics: relative inf-norm against the oracle


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(oracle_built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mp():
    import mp_block_preconditioners_amd as mp
    return mp


def _bits(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# (xi, eta_n, eta_s, c, d_u, d_p, d_div): the reference's parameters (every compile-time identity of the F policy and
# the unit pressure scalings taken), general ones (none taken), and c = 0 with eta_n = 1
PARAMS = [(1.0, 100.0, 1.0, 1.0, -1.0, 1.0, -1.0), (2.5, 1.0e4, 1.0, 0.5, -2.0, 0.5, -2.0),
          (1.0, 1.0, 1.0, 0.0, -1.0, 1.0, -1.0)]
PARAM_IDS = ["visc", "general", "c0"]
SIZES = [3, 4, 5, 17, 255, 256, 257, 300]
MODES = (0, 1, 2)   # SPMV_STORE, SPMV_ADD, SPMV_RESID


def _oracle_tables(n):
    from oracle.stokes_oracle import theta_tables
    return theta_tables(n)


@functools.lru_cache(maxsize=None)
def _system(n, prm):
    """(bp, assembled A, exact StokesOperator) over the oracle's thn tables: built once per (n, prm), never modified."""
    mp = _mp()
    xi, eta_n, eta_s, c, d_u, d_p, d_div = prm
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*_oracle_tables(n))
    A = bp.get_big_A_matrix(c=c, d_u=d_u, d_p=d_p, d_div=d_div)[0]
    return bp, A, bp.stokes_operator(c=c, d_u=d_u, d_p=d_p, d_div=d_div)


@functools.lru_cache(maxsize=None)
def _oracle_A(n, prm):
    from oracle.stokes_oracle import StokesSystem
    xi, eta_n, eta_s, c, d_u, d_p, d_div = prm
    return StokesSystem(n, xi, eta_n, eta_s, c, d_u, d_p=d_p, d_div=d_div, tables=_oracle_tables(n), products=False).A


@functools.lru_cache(maxsize=None)
def _vectors(n, seed):
    rng = np.random.default_rng(1000 * seed + n)
    return rng.standard_normal(5 * n * n), rng.standard_normal(5 * n * n)


@functools.lru_cache(maxsize=None)
def _oracle_Ax(n, prm, seed):
    from oracle import csr_oracle as co
    return co.spmv(_oracle_A(n, prm), _vectors(n, seed)[0])


@pytest.mark.parametrize("rows", [0, 1, 3, 8], ids=["auto", "march1", "march3", "march8"])
@pytest.mark.parametrize("prm", PARAMS, ids=PARAM_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_exact_bits(n, prm, rows):
    """Exact numerics equal the assembled A's CSR product in every mode and, at n <= 64, the sequential oracle's A u."""
    from mp_block_preconditioners_amd._lib import kernel_options
    _, A, op = _system(n, prm)
    assert op.shape == A.shape == (5 * n * n, 5 * n * n) and op.dtype == torch.float64 and op.device == A.device
    for seed in range(4 if n <= 5 else 1):   # few rows on the smallest grids: more vectors
        xh, zh = _vectors(n, seed)
        x, z = _cuda(xh), _cuda(zh)
        with kernel_options(march_rows=rows):
            got = [op.matvec(x, mode=m, z=z) for m in MODES]
        for m in MODES:
            want = A.matvec(x, mode=m, z=z)
            assert _bits(got[m], want), (n, seed, m, rel_inf(got[m].cpu().numpy(), want.cpu().numpy()))
        if n <= 64:
            ref = _oracle_Ax(n, prm, seed)
            assert _bits(got[0], ref), (n, seed, rel_inf(got[0].cpu().numpy(), ref))
            assert _bits(got[1], zh + ref) and _bits(got[2], zh - ref)


@pytest.mark.parametrize("prm", PARAMS[:2], ids=PARAM_IDS[:2])
@pytest.mark.parametrize("n", [17, 64, 257, 300])
def test_fast_numerics(n, prm):
    """Fast numerics: within 1e-12 relative inf-norm of the oracle's A u; pressure rows bit-identical to exact."""
    from oracle import csr_oracle as co
    bp, _, op = _system(n, prm)
    xi, eta_n, eta_s, c, d_u, d_p, d_div = prm
    fast = bp.stokes_operator(c=c, d_u=d_u, d_p=d_p, d_div=d_div, numerics="fast")
    assert fast.numerics == "fast" and fast.cell.data_ptr() == op.cell.data_ptr()
    rng = np.random.default_rng(n)
    x, z = rng.standard_normal(5 * n * n), rng.standard_normal(5 * n * n)
    ref = co.spmv(_oracle_A(n, prm), x)
    got = fast.matvec(_cuda(x))
    err = rel_inf(got.cpu().numpy(), ref)
    print(f"fast A u vs oracle, n = {n}, {prm}: {err:.3e}")
    assert err <= TOL_FAST, err
    exact = op.matvec(_cuda(x))
    N = n * n
    assert torch.equal(got[4 * N:], exact[4 * N:])
    for m in (1, 2):
        gm, em = fast.matvec(_cuda(x), mode=m, z=_cuda(z)), op.matvec(_cuda(x), mode=m, z=_cuda(z))
        want = z + ref if m == 1 else z - ref
        assert np.max(np.abs(gm.cpu().numpy() - want)) <= TOL_FAST * np.max(np.abs(ref))
        assert torch.equal(gm[4 * N:], em[4 * N:])


def _shifted_tables(n):
    """Another smooth field, 0.5 + 0.3 cos(2 pi (x + 0.1)) sin(4 pi (y - 0.2)), at the three tables' points."""
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * (x + 0.1)) * np.sin(4 * np.pi * (y - 0.2))
    return f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx)


@pytest.mark.parametrize("how", ["set_params", "refill"])
def test_time_step(how):
    """New thn values, xi, eta and coefficients reach the operator in place: it equals a freshly assembled A."""
    mp = _mp()
    n = 96
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    bp.set_theta_tables(*_oracle_tables(n))
    op = bp.get_big_A_matrix(c=1.0, d_u=-1.0, matrix_free_A=True)[0]
    assert isinstance(op, mp.StokesOperator)
    x = _cuda(np.random.default_rng(5).standard_normal(5 * n * n))
    before = op.matvec(x)
    addrs = (op.cell.data_ptr(), op.uface.data_ptr(), op.vface.data_ptr())
    bp.update_theta_tables(*_shifted_tables(n))
    bp.xi, bp.eta_n, bp.eta_s = 2.5, 40.0, 3.0
    new = dict(c=0.5, d_u=-2.0, d_p=0.5, d_div=-2.0)
    if how == "set_params":
        op.set_params(xi=bp.xi, eta_n=bp.eta_n, eta_s=bp.eta_s, **new)
    else:
        bp.refill(op, None, None, None, **new)
    assert (op.cell.data_ptr(), op.uface.data_ptr(), op.vface.data_ptr()) == addrs
    fresh = bp.get_big_A_matrix(**new)[0]
    got = op.matvec(x)
    assert _bits(got, fresh.matvec(x))
    assert not torch.equal(got, before)
    # refill refuses an operator over tables this object no longer holds, before anything is written
    bp.set_theta_tables(*_oracle_tables(n))
    with pytest.raises(ValueError):
        bp.refill(op, None, None, None, **new)


def test_solver_same_iterates():
    """FGMRES with the operator in A's place: same info, iterates and residual history as with the assembled A."""
    mp = _mp()
    n = 32
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    op = bp.stokes_operator(c=1.0, d_u=-1.0)
    pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("chebyshev", 5),
                                      inner_P=mp.InnerSolver("chebyshev", 5))
    u_vec, b_vec = mp.manufactured_problem(n, xi=1.0, etan=100.0, etas=1.0)
    b = _cuda(b_vec)
    runs = []
    for M in (A, op):
        hist, iterates = [], []
        x, info = mp.fgmres(M, b, M=pc, tol=1e-8, residuals=hist, callback=lambda xk: iterates.append(xk.clone()))
        runs.append((x, info, hist, iterates))
    (xa, ia, ha, ita), (xo, io, ho, ito) = runs
    assert ia == io and ha == ho and len(ha) > 1
    assert torch.equal(xa, xo) and len(ita) == len(ito) and all(torch.equal(p, q) for p, q in zip(ita, ito))
    # the reference-shaped entry point end to end, A never assembled
    kw = dict(inner_F=mp.InnerSolver("chebyshev", 5), inner_P=mp.InnerSolver("chebyshev", 5), verbose=False)
    ua, infa, hista = mp.solve_with_approx_schur_pc(n, 1.0, 100.0, 1.0, 1.0, -1.0, b_vec, u_vec, **kw)
    uo, info, histo = mp.solve_with_approx_schur_pc(n, 1.0, 100.0, 1.0, 1.0, -1.0, b_vec, u_vec, matrix_free_A=True,
                                                    **kw)
    assert infa == info and hista == histo and _bits(ua, uo)
    uw, infw, histw = mp.solve_without_pc(n, op, b_vec, u_vec, tol=1e-2, maxiter=20, verbose=False)
    ux, infx, histx = mp.solve_without_pc(n, A, b_vec, u_vec, tol=1e-2, maxiter=20, verbose=False)
    assert infw == infx and histw == histx and _bits(uw, ux)


def test_graph_capture():
    """One apply captured into a graph on a side stream and replayed equals the eager result: a single kernel node."""
    n = 64
    _, _, op = _system(n, PARAMS[0])
    x = _cuda(_vectors(n, 0)[0])
    eager = op.apply(x)
    y = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op.apply(x, out=y)                     # warm-up on the side stream, as torch requires
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            op.apply(x, out=y)
    torch.cuda.current_stream().wait_stream(side)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    x.mul_(2.0)                                # the graph reads x by address: power-of-two scaling is exact
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, 2.0 * eager)


def test_refusals_and_host_vectors():
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    small = mp.MultiphaseBlockPreconditioner(2, 1.0, 1.0, 1.0)
    with pytest.raises(ValueError):
        small.stokes_operator(c=1.0, d_u=-1.0)
    with pytest.raises(ValueError):
        small.get_big_A_matrix(c=1.0, d_u=-1.0, matrix_free_A=True)
    assert isinstance(small.get_big_A_matrix(c=1.0, d_u=-1.0)[0], mp.DeviceCSR)   # the default is untouched
    with pytest.raises(ValueError):
        mp.StokesOperator(small._params(), small.theta_tables())
    n = 5
    bp, A, op = _system(n, PARAMS[0])
    with pytest.raises(ValueError):
        bp.stokes_operator(c=1.0, d_u=-1.0, numerics="bogus")
    m = 5 * n * n
    x = _cuda(_vectors(n, 0)[0])
    with pytest.raises(ValueError):
        op.matvec(x[:-1])
    with pytest.raises(ValueError):
        op.matvec(x, out=torch.empty(m - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        op.matvec(x.cpu())
    with pytest.raises(mp.MpbpError):
        op.matvec(x, out=x)
    with pytest.raises(mp.MpbpError):
        op.matvec(x, mode=_lib.SPMV_ADD)
    with pytest.raises(mp.MpbpError):
        op.matvec(x, mode=7)
    xh = _vectors(n, 0)[0]
    for bad in (xh[:-1], np.concatenate([xh, xh[:1]])):
        with pytest.raises(ValueError, match="dimension mismatch"):
            op @ bad
    yh = op @ xh
    assert isinstance(yh, np.ndarray) and _bits(yh, (op @ x).cpu())
    assert _bits(yh, A @ xh)
    op.release_staging()
