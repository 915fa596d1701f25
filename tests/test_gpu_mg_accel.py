"""Chebyshev acceleration of the multigrid V-cycles (InnerSolver("mg", K, accel="chebyshev"), mpbp_mg_combine,
mpbp_mg_accel_coeffs) on the GPU against the numpy restatement (tests/mg_accel_restatement.py over
oracle/mg_oracle.py's V-cycle): exact numerics bit for bit, fast numerics at the project's conditioning-floor rule."""
import ctypes
import functools

import numpy as np
import pytest

import mg_accel_restatement as ar
from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_APPLY = 1e-12   # north_star's fp64 bar; the fast apply is held to max(TOL_APPLY, 4 x the one-ulp floor)
UNIT = (1.0, 100.0, 1.0, 1.0, -1.0)        # xi, eta_n, eta_s, c, d_u
GENERAL = (2.5, 37.0, 0.6, 0.8, -1.7)
PRMS = {"unit": UNIT, "general": GENERAL}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(oracle_built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mp():
    import mp_block_preconditioners_amd as mp
    return mp


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _oracle_system(n, prm):
    from oracle.stokes_oracle import StokesSystem, theta_tables
    xi, eta_n, eta_s, c, d_u = prm
    tabs = theta_tables(n)
    return tabs, StokesSystem(n, xi, eta_n, eta_s, c, d_u, tables=tabs)


def _system(n, prm=UNIT):
    """(bp, (A, F, D, G) on the GPU, the oracle's StokesSystem) on the same thn tables."""
    mp = _mp()
    xi, eta_n, eta_s, c, d_u = prm
    tabs, S = _oracle_system(n, prm)
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*tabs)
    A, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u)
    return bp, (A, F, D, G), S


def _oracle_of(mg, Mh):
    """oracle/mg_oracle.py's hierarchy with the GPU hierarchy's smoothing bounds and coarse inverse."""
    from oracle import mg_oracle as mo
    return mo.MgOracle(Mh, mg.n, mg.fields, mg.pre, mg.post, 1, bounds=mg.bounds, coarse_inv=mg.coarse_inv_host,
                       coarsest=mg.coarsest)


# ------------------------------------------------------------------------------------ 1. the two entry points
def _combine(n, y, xk, xold, omega, mu, sub, out):
    from mp_block_preconditioners_amd._lib import check, lib, ptr, stream_handle
    check(lib().mpbp_mg_combine(n, ptr(y), ptr(xk), ptr(xold), omega, mu, ptr(sub), ptr(out), stream_handle()))


# 36 865: several workgroups and an odd tail; 1 048 579: more 16-byte pairs than the grid's 2048 x 256 lanes, so the
# grid-stride loop runs a second time (and the element-wise path's too)
LENGTHS = [1, 63, 64, 65, 400, 36865, 1048579]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", LENGTHS)
def test_combine_bit_identical_to_numpy(n, offset):
    """Every form (k = 0; k = 1 with x_0 = 0 not read; k >= 2), with and without sub, out separate and out aliasing
    xold, on 16-byte-aligned vectors and with every pointer offset by one element (the element-wise path)."""
    rng = np.random.default_rng(n + offset)
    host = {k: rng.standard_normal(n + 1) for k in ("y", "xk", "xold", "sub")}
    omega, mu = 1.0526315789473684, 0.0007304601899196494

    def dev(a):
        t = _cuda(a)
        assert t.data_ptr() % 16 == 0
        v = t[offset:offset + n]
        assert v.data_ptr() % 16 == (8 * offset) % 16
        return v
    h = {k: a[offset:offset + n] for k, a in host.items()}
    zeros = np.zeros(n)
    for form in ("first", "second", "full"):
        for use_sub in (False, True):
            for alias in ((False, True) if form == "full" else (False,)):
                d = {k: dev(host[k]) for k in host}
                xk = None if form == "first" else d["xk"]
                xold = d["xold"] if form == "full" else None
                out = xold if alias else dev(np.full(n + 1, np.nan))
                _combine(n, d["y"], xk, xold, omega, mu, d["sub"] if use_sub else None, out)
                ref = ar.combine(h["y"], None if form == "first" else h["xk"], h["xold"] if form == "full" else zeros,
                                 omega, mu, h["sub"] if use_sub else None)
                assert np.array_equal(_bits(out), _bits(ref)), (form, use_sub, alias)
                # the operands are only read (out apart)
                for k in ("y", "xk", "sub") + (() if alias else ("xold",)):
                    assert np.array_equal(_bits(d[k]), _bits(h[k])), k
    # one pointer off the 16-byte grid among aligned ones: the element-wise path, same bits
    if offset == 0 and n > 1:
        y1 = _cuda(host["y"])[1:n]
        out = dev(np.full(n + 1, np.nan))[: n - 1]
        _combine(n - 1, y1, dev(host["xk"])[: n - 1], dev(host["xold"])[: n - 1], omega, mu, None, out)
        ref = ar.combine(host["y"][1:n], host["xk"][: n - 1], host["xold"][: n - 1], omega, mu)
        assert np.array_equal(_bits(out), _bits(ref))


def test_combine_rejects_bad_arguments():
    from mp_block_preconditioners_amd._lib import MpbpError
    y, out = _cuda(np.ones(8)), _cuda(np.zeros(8))
    with pytest.raises(MpbpError):
        _combine(8, y, None, y, 1.0, 0.0, None, out)    # xold without xk
    with pytest.raises(MpbpError):
        _combine(8, None, None, None, 1.0, 0.0, None, out)
    _combine(0, None, None, None, 1.0, 0.0, None, None)  # nothing to do


def test_accel_coeffs_bit_identical_to_restatement():
    from mp_block_preconditioners_amd._lib import lib
    L = lib()
    for rho in (0.05, 0.0998, 0.1, 0.375, 0.499, 0.9):
        for K in (1, 2, 3, 8, 64):
            om, mu = np.full(K, np.nan), np.full(K, np.nan)
            assert L.mpbp_mg_accel_coeffs(rho, K, om.ctypes.data_as(ctypes.c_void_p),
                                          mu.ctypes.data_as(ctypes.c_void_p)) == 0
            ro, rm = ar.accel_coeffs(rho, K)
            assert np.array_equal(_bits(om), _bits(np.array(ro))) and np.array_equal(_bits(mu), _bits(np.array(rm)))
    c = np.zeros(65)
    p = c.ctypes.data_as(ctypes.c_void_p)
    for rho, K in ((0.1, 0), (0.1, 65), (0.0, 3), (1.0, 3), (-0.1, 3), (float("nan"), 3)):
        assert L.mpbp_mg_accel_coeffs(rho, K, p, p) == -1, (rho, K)
    assert b"mg_accel_coeffs" in L.mpbp_last_error()


# ------------------------------------------------------------------------------------ 2. the standalone solve
@pytest.mark.parametrize("sell", [True, False], ids=["sell", "csr"])
@pytest.mark.parametrize("which,n", [("F", 16), ("F", 32), ("F", 64), ("GtG", 32)])
def test_mg_solve_accel_bit_exact(which, n, sell):
    """Multigrid.solve, exact numerics, vs the restatement for K = 1, 2, 3, 5 (K = 1: omega_0 y alone; 2: the step that
    does not read x_0; 3, 5: both accel_x buffers in turn), with and without sub.  F: rho estimated; Gt_G (singular): the
    explicit rho = 0.1 and a zero-mean right-hand side."""
    mp = _mp()
    _, (A, F, D, G), S = _system(n)
    if which == "F":
        M, Mh, fields, rho = F, S.F, mp.FIELDS_VELOCITY, None
    else:
        M, _ = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)
        Mh, fields, rho = S.GtG, mp.FIELDS_PRESSURE, 0.1
    rng = np.random.default_rng(100 * n + sell)
    b = rng.standard_normal(M.shape[0])
    b -= b.mean()
    sub = rng.standard_normal(M.shape[0])
    for K in (1, 2, 3, 5):
        mg = mp.Multigrid(M, n, fields, cycles=K, sell=sell, accel="chebyshev", rho=rho)
        if rho is None:
            rho = mg.rho      # estimated once: the later hierarchies take it as given (the same operator)
            assert mg.rho_estimated and 0.0 < rho < 0.5
        assert mg.rho == rho
        vc = ar.oracle_vcycle(_oracle_of(mg, Mh))
        got = mg.solve(_cuda(b))
        assert np.array_equal(_bits(got), _bits(ar.accel_solve(vc, b, K, rho))), K
        got = mg.solve(_cuda(b), sub=_cuda(sub))
        assert np.array_equal(_bits(got), _bits(ar.accel_solve(vc, b, K, rho, sub=sub))), K
        # accel=None on the same operator is the stationary iteration, untouched
        if K == 3:
            plain = mp.Multigrid(M, n, fields, cycles=K, sell=sell)
            assert plain.rho is None and plain.accel_x is None
            assert np.array_equal(_bits(plain.solve(_cuda(b))), _bits(ar.stationary_solve(vc, b, K)))


def test_partitioned_hierarchy_refuses_acceleration():
    """part_levels > 0 with accel: MPBP_ERR_ARG before anything is launched or any callback called."""
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    _, (A, F, D, G), _ = _system(16)
    mg = mp.Multigrid(F, 16, mp.FIELDS_VELOCITY, cycles=2, accel="chebyshev", rho=0.1)
    called = []
    halo = _lib.HALO_FN(lambda *a: called.append("halo"))
    gather = _lib.GATHER_FN(lambda *a: called.append("gather"))
    mg._mg.part_levels, mg._mg.halo, mg._mg.gather = 1, halo, gather
    try:
        with pytest.raises(_lib.MpbpError, match="row-partitioned"):
            mg.solve(_cuda(np.ones(F.shape[0])))
    finally:
        mg._mg.part_levels, mg._mg.halo, mg._mg.gather = 0, _lib.HALO_FN(), _lib.GATHER_FN()
    assert not called


# ------------------------------------------------------------------------------------ 3. inside the Schur apply
K_F, RHO = 3, 0.1


def _inner(mp):
    return dict(inner_F=mp.InnerSolver("mg", K_F, accel="chebyshev", rho=RHO), inner_P=mp.InnerSolver("mg", 1))


def _oracle_apply(S, pc, v):
    """approx_schur_op (solve.py:257-277): F^-1 the accelerated cycles, Gt_G^-1 one plain cycle."""
    from oracle import csr_oracle as co
    vF = ar.oracle_vcycle(_oracle_of(pc.mg_F, S.F))
    oP = _oracle_of(pc.mg_P, S.GtG)
    nu = S.F.shape[0]
    Finv_v = ar.accel_solve(vF, v[:nu], K_F, RHO)
    rhs = co.spmv(S.D, Finv_v, v[nu:], mode=1)
    x_a = oP.solve(rhs)
    x_b = co.spmv(S.GtFG, x_a)
    x_p = oP.solve(x_b)
    u = ar.accel_solve(vF, co.spmv(S.G, x_p), K_F, RHO, sub=Finv_v)
    return np.concatenate([u, x_p])


@pytest.mark.parametrize("prm", ["unit", "general"])
@pytest.mark.parametrize("n", [16, 64, 96])
def test_schur_apply_accel_bit_exact(n, prm):
    """Exact numerics vs the oracle apply; n = 96 is where level 0's fused launches run (tests/test_gpu_refresh.py)."""
    mp = _mp()
    _, (A, F, D, G), S = _system(n, PRMS[prm])
    pc = mp.ApproxSchurPreconditioner(F, D, G, **_inner(mp))
    assert pc.mg_F.accel == "chebyshev" and pc.mg_F.rho == RHO and not pc.mg_F.rho_estimated and pc.mg_P.accel is None
    v = np.random.default_rng(n).standard_normal(pc.shape[0])
    got = pc.apply(_cuda(v))
    assert np.array_equal(_bits(got), _bits(_oracle_apply(S, pc, v)))


@pytest.mark.parametrize("prm", ["unit", "general"])
@pytest.mark.parametrize("n", [64, 96])
def test_schur_apply_accel_fast_at_the_conditioning_floor(n, prm):
    """Fast numerics against the exact GPU apply (the oracle's bits, above): within max(1e-12, 4 x floor), the floor
    measured as tests/test_gpu_fast.py measures it -- the exact apply of the input changed by one ulp per entry.
    Measured (MI355X, profiles/mg_accel_measured.txt): err 2.6e-14 .. 1.0e-13, floors 1.3e-14 .. 3.6e-14."""
    mp = _mp()
    _, (A, F, D, G), _ = _system(n, PRMS[prm])
    fast = mp.ApproxSchurPreconditioner(F, D, G, numerics="fast", **_inner(mp))
    exact = mp.ApproxSchurPreconditioner(F, D, G, fast.GtG, fast.GtFG, **_inner(mp))
    rng = np.random.default_rng(7 * n)
    v = rng.standard_normal(fast.shape[0])
    v_ulp = v * (1.0 + np.where(rng.random(v.size) < 0.5, -1.0, 1.0) * 2.0 ** -52)
    ref = exact.apply(_cuda(v)).cpu().numpy()
    floor = rel_inf(exact.apply(_cuda(v_ulp)).cpu().numpy(), ref)
    err = rel_inf(fast.apply(_cuda(v)).cpu().numpy(), ref)
    print(f"mg_accel fast vs exact: n={n} {prm}: err {err:.3e}, one-ulp floor {floor:.3e}, "
          f"bound {max(TOL_APPLY, 4.0 * floor):.3e}")
    assert floor > 0.0
    assert err <= max(TOL_APPLY, 4.0 * floor), (err, floor)


# ------------------------------------------------------------------------------------ 4. graph capture
@pytest.mark.parametrize("n,numerics", [(64, "exact"), (96, "exact"), (96, "fast")])
def test_captured_apply_equals_eager(n, numerics):
    mp = _mp()
    _, (A, F, D, G), _ = _system(n)
    pc = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics, **_inner(mp))
    v = _cuda(np.random.default_rng(n).standard_normal(pc.shape[0]))
    eager = pc.apply(v).clone()
    out = torch.full_like(v, float("nan"))
    g = pc.capture(v, out)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, eager) and torch.equal(out, first)


# ------------------------------------------------------------------------------------ 5. the estimator
def test_contraction_and_rho_match_the_restatement():
    """The power iteration's vectors are the restatement's bit for bit, so the ratios differ only by the norm's
    summation order (1e-10 relative is orders above that); rho is 1.1 x the largest of the last three, exactly."""
    mp = _mp()
    from mp_block_preconditioners_amd import mg as mgmod
    n = 32
    _, (A, F, D, G), S = _system(n)
    mg = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, cycles=3, coarsest=16, accel="chebyshev")
    ratios = mg.contraction()
    assert len(ratios) == 8 and len(mg.contraction(steps=3)) == 3
    ref, _ = ar.contraction(S.F, ar.oracle_vcycle(_oracle_of(mg, S.F)))
    assert np.max(np.abs(np.array(ratios) / np.array(ref) - 1.0)) <= 1e-10, (ratios, ref)
    assert mgmod.ACCEL_RHO_MARGIN == 1.1
    assert mg.rho == 1.1 * max(ratios[-3:]) and mg.rho_estimated
    assert mg.cstruct().accel_rho == mg.rho and mg.cstruct().cycles == 3 and mg.cstruct().accel == 1
    assert mg.contraction(seed=1) != ratios
    # an explicit rho is used as given
    given = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, cycles=3, coarsest=16, accel="chebyshev", rho=0.2)
    assert given.rho == 0.2 and not given.rho_estimated and given.cstruct().accel_rho == 0.2


def test_singular_operators_are_refused():
    """Gt_G, and F assembled with c = 0: the null space gives I - M A an eigenvalue of 1, the estimate is >= 0.5."""
    mp = _mp()
    n = 32
    _, (A, F, D, G), _ = _system(n)
    GtG, _ = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)
    with pytest.raises(ValueError, match="rho = "):
        mp.Multigrid(GtG, n, mp.FIELDS_PRESSURE, accel="chebyshev")
    _, (_, F0, _, _), _ = _system(n, (1.0, 100.0, 1.0, 0.0, -1.0))
    with pytest.raises(ValueError, match="rho = "):
        mp.Multigrid(F0, n, mp.FIELDS_VELOCITY, accel="chebyshev")
    with pytest.raises(ValueError, match="rho = "):
        mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("mg", 2),
                                     inner_P=mp.InnerSolver("mg", 2, accel="chebyshev"))


# ------------------------------------------------------------------------------------ 6. refresh
@pytest.mark.parametrize("n,numerics", [(32, "exact"), (96, "fast")])
def test_refresh_matches_a_fresh_preconditioner(n, numerics):
    """update_theta_tables + refill + refresh with changed thn, eta and c: the accelerated apply and the re-estimated
    rho are a freshly built preconditioner's, bit for bit."""
    mp = _mp()
    from oracle.stokes_oracle import theta_tables
    inner = dict(inner_F=mp.InnerSolver("mg", 3, accel="chebyshev"), inner_P=mp.InnerSolver("mg", 1))
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * x) * np.sin(4 * np.pi * y)
    new_tabs = (f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx))
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    bp.set_theta_tables(*theta_tables(n))
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    pc = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics, **inner)
    rho0 = pc.mg_F.rho
    bp.update_theta_tables(*new_tabs)
    bp.eta_n = 1.0e4
    bp.refill(A, F, D, G, c=4.0, d_u=-1.0)
    timings = {}
    pc.refresh(timings=timings)
    assert "accel_rho" in timings and timings["accel_rho"] > 0.0
    bp2 = mp.MultiphaseBlockPreconditioner(n, 1.0, 1.0e4, 1.0)
    bp2.set_theta_tables(*new_tabs)
    _, _, F2, D2, G2 = bp2.get_big_A_matrix(c=4.0, d_u=-1.0)
    fresh = mp.ApproxSchurPreconditioner(F2, D2, G2, numerics=numerics, **inner)
    assert pc.mg_F.rho == fresh.mg_F.rho and pc.mg_F.rho != rho0
    assert pc.mg_F.cstruct().accel_rho == fresh.mg_F.rho
    v = _cuda(np.random.default_rng(n).standard_normal(pc.shape[0]))
    assert torch.equal(pc.apply(v), fresh.apply(v))


# ------------------------------------------------------------------------------------ 7. the effect
def test_accelerated_residual_at_64():
    """n = 64, eta_n = 100, exact numerics, V(2,2), coarsest 16: the F residual after 4 accelerated cycles is below
    0.2 x that of 4 stationary ones (CPU oracle: 0.077 x, 8.5e-7 against 1.1e-5; the GPU computes its bits)."""
    mp = _mp()
    n = 64
    _, (A, F, D, G), _ = _system(n)
    b = _cuda(np.random.default_rng(0).standard_normal(F.shape[0]))
    res = {}
    for accel in (None, "chebyshev"):
        mg = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, cycles=4, coarsest=16, accel=accel)
        x = mg.solve(b)
        res[accel] = float(torch.linalg.vector_norm(b - F.matvec(x)) / torch.linalg.vector_norm(b))
    print(f"F residual after 4 cycles at 64^2: stationary {res[None]:.3e}, accelerated {res['chebyshev']:.3e}")
    assert res["chebyshev"] < 0.2 * res[None], res
