"""The upper, lower and diagonal block forms of the Schur preconditioner (ApproxSchurPreconditioner(form=...),
mpbp_schur_plan.form) on the GPU: exact numerics bit for bit against tests/block_forms_restatement.py, the upper form's
right-hand side v_u - G x_p built inside the whole F solve launch (GxR, plan.fuse_g) against the G launch + solve pair,
fast numerics at the project's conditioning-floor rule, and the forms under capture, refresh, refusals and FGMRES."""
import ctypes
import functools

import numpy as np
import pytest

import block_forms_restatement as bf
from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_APPLY = 1e-12   # north_star's fp64 bar; a fast apply is held to max(TOL_APPLY, 4 x the one-ulp floor)
UNIT = (1.0, 100.0, 1.0, 1.0, -1.0)        # xi, eta_n, eta_s, c, d_u
GENERAL = (2.5, 37.0, 0.6, 0.8, -1.7)
STIFF = (1.0, 1.0e4, 1.0, 1.0, -1.0)       # the eta ratio 1e4 set
PRMS = {"unit": UNIT, "general": GENERAL, "stiff": STIFF}
NEW_FORMS = ("upper", "lower", "diagonal")
RHO = 0.1


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
    """(A, F, D, G) on the GPU and the oracle's StokesSystem on the same thn tables."""
    mp = _mp()
    xi, eta_n, eta_s, c, d_u = prm
    tabs, S = _oracle_system(n, prm)
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*tabs)
    A, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u)
    return (A, F, D, G), S


def _oracle_of(mg, Mh):
    from oracle import mg_oracle as mo
    return mo.MgOracle(Mh, mg.n, mg.fields, mg.pre, mg.post, mg.cycles, bounds=mg.bounds,
                       coarse_inv=mg.coarse_inv_host, coarsest=mg.coarsest)


INNER = {"cheb43": lambda mp: (mp.InnerSolver("chebyshev", 4), mp.InnerSolver("chebyshev", 3)),
         "jacobi32": lambda mp: (mp.InnerSolver("jacobi", 3), mp.InnerSolver("jacobi", 2)),
         "mg11": lambda mp: (mp.InnerSolver("mg", 1), mp.InnerSolver("mg", 1)),
         "accel3": lambda mp: (mp.InnerSolver("mg", 3, accel="chebyshev", rho=RHO), mp.InnerSolver("mg", 1))}


def _restated_solvers(pc, S):
    """The restatement's inner solves with the preconditioner's own intervals, hierarchies and rho."""
    from oracle.schur_oracle import Inner

    def one(inner, mg, Mh):
        if inner.kind == "mg":
            ora = _oracle_of(mg, Mh)
            return bf.mg_accel_solver(ora, inner.sweeps, mg.rho) if mg.accel else bf.mg_solver(ora)
        return Inner(inner.kind, inner.sweeps, inner.lmin, inner.lmax)
    return one(pc.inner_F, pc.mg_F, S.F), one(pc.inner_P, pc.mg_P, S.GtG)


# ------------------------------------------------------------------------------------ 1. exact numerics, bit for bit
def _exact_case(n, prm, inner, **kw):
    mp = _mp()
    (A, F, D, G), S = _system(n, PRMS[prm])
    iF, iP = INNER[inner](mp)
    v = np.random.default_rng(31 * n + len(inner)).standard_normal(5 * n * n)
    first = solvers = None
    for form in NEW_FORMS:
        args = (F, D, G) if first is None else (F, D, G, first.GtG, first.GtFG)
        pc = mp.ApproxSchurPreconditioner(*args, inner_F=iF, inner_P=iP, form=form, **kw)
        assert pc.form == form and pc._plan.form == mp.FORMS.index(form)
        assert pc.fuse_g == (form == "upper" and iF.kind == "chebyshev" and pc.f_stencil is not None
                             and pc.pg_stencil is not None)
        if first is None:
            first, solvers = pc, _restated_solvers(pc, S)
        want = bf.apply(form, S.F, S.D, S.G, S.GtG, S.GtFG, v, *solvers)
        got = pc.apply(_cuda(v))
        assert np.array_equal(_bits(got), _bits(want)), (form, rel_inf(got.cpu().numpy(), want))
    return first


# n = 5 has no multigrid hierarchy to compare: an odd grid does not coarsen under coarsen="even" (mg.level_sizes), and
# oracle/mg_oracle.py restates no other coarsening -- the sweeping solvers cover the smallest diamond
EXACT_CASES = [(n, inner) for n in (5, 16, 64, 96) for inner in INNER if not (n == 5 and inner in ("mg11", "accel3"))]


@pytest.mark.parametrize("prm", ["unit", "general"])
@pytest.mark.parametrize("n,inner", EXACT_CASES)
def test_exact_apply_bit_identical_to_the_restatement(n, inner, prm):
    """n = 5: the smallest diamond; 16, 64; 96 where every fused launch of the apply is taken
    (tests/test_gpu_refresh.py)."""
    _exact_case(n, prm, inner)


@pytest.mark.parametrize("kw", [dict(layout="csr"), dict(f_mode="assembled", pg_mode="assembled")],
                         ids=["csr", "assembled"])
@pytest.mark.parametrize("inner", list(INNER))
@pytest.mark.parametrize("prm", ["unit", "general"])
def test_exact_apply_other_layouts(prm, inner, kw):
    pc = _exact_case(16, prm, inner, **kw)
    if "f_mode" in kw:
        assert pc.f_stencil is None and pc.pg_stencil is None


@pytest.mark.parametrize("numerics", ["exact", "fast"])
def test_full_given_explicitly_is_the_default(numerics):
    mp = _mp()
    (A, F, D, G), _ = _system(96)
    v = _cuda(np.random.default_rng(3).standard_normal(5 * 96 * 96))
    default = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics)
    full = mp.ApproxSchurPreconditioner(F, D, G, default.GtG, default.GtFG, numerics=numerics, form="full")
    assert default.form == full.form == "full" and default._plan.form == 0 and full.fuse_g == default.fuse_g
    assert torch.equal(full.apply(v), default.apply(v))


# ------------------------------------------------------------------------------------ 2. the fused right-hand side
def _fsolve_ok(K, n):
    """launch_fsolve's gate (csrc/f_solve_w.inc fsolve_ok): the 64 x 8 tile's staged window, tile + K each side."""
    return K in (3, 4) and n >= 64 + 2 * K


@pytest.mark.parametrize("kf", [3, 4])
@pytest.mark.parametrize("prm", ["unit", "general", "stiff"])
@pytest.mark.parametrize("n", [64, 70, 72, 73, 81, 96, 257])
def test_fused_rhs_equals_the_g_launch_and_solve(n, prm, kf):
    """Fast numerics, form="upper": the whole-solve launch that builds v_u - G x_p per cell (fuse_g) against the G
    launch in MPBP_SPMV_RESID mode followed by the solve -- the same bits, on both tiles and on the marching fallback.
    That the fused launch ran is read from the plan: it records ONE profiled F launch and never writes the plan's W
    buffer (wu_owned), which the pair fills."""
    mp = _mp()
    (A, F, D, G), _ = _system(n, PRMS[prm])
    kw = dict(inner_F=mp.InnerSolver("chebyshev", kf), inner_P=mp.InnerSolver("chebyshev", 4), numerics="fast",
              form="upper")
    fused = mp.ApproxSchurPreconditioner(F, D, G, fuse_g=True, **kw)
    apart = mp.ApproxSchurPreconditioner(F, D, G, fused.GtG, fused.GtFG, fuse_g=False, **kw)
    assert fused.fuse_g and not apart.fuse_g and fused._plan.fuse_g == 1 and apart._plan.fuse_g == 0
    v = _cuda(np.random.default_rng(100 * n + kf).standard_normal(fused.shape[0]))
    want = apart.apply(v).clone()
    assert bool(torch.isfinite(want).all())
    takes = _fsolve_ok(kf, n)
    for opts in (dict(), dict(f_solve_tile=0), dict(f_solve=0)):
        fused.set_kernel_opts(f_solve=1, f_solve_tile=1)
        fused.set_kernel_opts(**opts)
        fused.enable_profiling(16)
        fused._wu_owned.fill_(float("nan"))
        got = fused.apply(v)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (opts, float((got - want).abs().max()))
        w_untouched = bool(torch.isnan(fused._wu_owned).all())
        if takes and opts.get("f_solve", 1):
            assert w_untouched and len(fused.profiled_ms()) == 1, opts
        else:   # the pair: W = v_u - G x_p was stored
            assert bool(torch.isfinite(fused._wu_owned).all()), opts
    assert bool(torch.isfinite(apart._wu_owned).all())


# ------------------------------------------------------------------------------------ 3. fast against exact
@pytest.mark.parametrize("inner", ["cheb44", "mg11"])
@pytest.mark.parametrize("prm", ["unit", "general"])
@pytest.mark.parametrize("n", [64, 96])
def test_fast_apply_at_the_conditioning_floor(n, prm, inner):
    """Fast numerics against the exact GPU apply of the same form (the restatement's bits, section 1): within
    max(1e-12, 4 x floor), the floor measured as tests/test_gpu_fast.py measures it -- the exact apply of the input
    changed by one ulp per entry.  Measured (MI355X, profiles/block_forms_measured.txt): chebyshev:4 / chebyshev:4 err
    9.8e-16 .. 1.6e-15 with floors 1.1e-15 .. 2.1e-15; mg:1 / mg:1 err 1.6e-14 .. 6.9e-14 with floors 1.1e-14 .. 5.2e-14
    (the largest ratio err / floor 2.4, upper and diagonal at n = 96, unit parameters)."""
    mp = _mp()
    (A, F, D, G), _ = _system(n, PRMS[prm])

    def inners():
        if inner == "mg11":
            return dict(inner_F=mp.InnerSolver("mg", 1), inner_P=mp.InnerSolver("mg", 1))
        return dict(inner_F=mp.InnerSolver("chebyshev", 4), inner_P=mp.InnerSolver("chebyshev", 4))
    rng = np.random.default_rng(7 * n)
    v = rng.standard_normal(5 * n * n)
    v_ulp = v * (1.0 + np.where(rng.random(v.size) < 0.5, -1.0, 1.0) * 2.0 ** -52)
    products = None
    for form in NEW_FORMS:
        args = (F, D, G) if products is None else (F, D, G, *products)
        fast = mp.ApproxSchurPreconditioner(*args, numerics="fast", form=form, **inners())
        products = (fast.GtG, fast.GtFG)
        exact = mp.ApproxSchurPreconditioner(F, D, G, *products, form=form, **inners())
        ref = exact.apply(_cuda(v)).cpu().numpy()
        floor = rel_inf(exact.apply(_cuda(v_ulp)).cpu().numpy(), ref)
        err = rel_inf(fast.apply(_cuda(v)).cpu().numpy(), ref)
        print(f"block forms fast vs exact: {form} {inner} n={n} {prm}: err {err:.3e}, one-ulp floor {floor:.3e}, "
              f"bound {max(TOL_APPLY, 4.0 * floor):.3e}")
        assert floor > 0.0
        assert err <= max(TOL_APPLY, 4.0 * floor), (form, err, floor)


# ------------------------------------------------------------------------------------ 4. relations between the forms
@pytest.mark.parametrize("numerics", ["exact", "fast"])
def test_forms_share_their_pressure_parts(numerics):
    """lower's x_p is full's and diagonal's is upper's, bit for bit; lower's and diagonal's u are one F solve of v_u."""
    mp = _mp()
    n = 96
    (A, F, D, G), _ = _system(n)
    nu = F.shape[0]
    v = _cuda(np.random.default_rng(11).standard_normal(5 * n * n))
    out, products = {}, ()
    for form in mp.FORMS:
        pc = mp.ApproxSchurPreconditioner(F, D, G, *products, numerics=numerics, form=form)
        products = (pc.GtG, pc.GtFG)
        out[form] = pc.apply(v).clone()
    assert torch.equal(out["lower"][nu:], out["full"][nu:])
    assert torch.equal(out["diagonal"][nu:], out["upper"][nu:])
    assert torch.equal(out["diagonal"][:nu], out["lower"][:nu])
    assert not torch.equal(out["upper"][nu:], out["full"][nu:]) and not torch.equal(out["upper"][:nu], out["lower"][:nu])


# ------------------------------------------------------------------------------------ 5. graph capture
@pytest.mark.parametrize("form", NEW_FORMS)
@pytest.mark.parametrize("n,numerics", [(96, "fast"), (64, "exact")])
def test_captured_apply_equals_eager(n, numerics, form):
    mp = _mp()
    (A, F, D, G), _ = _system(n)
    pc = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics, form=form)
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


# ------------------------------------------------------------------------------------ 6. refresh
@pytest.mark.parametrize("form", NEW_FORMS)
@pytest.mark.parametrize("n,numerics", [(32, "exact"), (96, "fast")])
def test_refresh_matches_a_fresh_preconditioner(n, numerics, form):
    """update_theta_tables + refill + refresh with changed thn, eta and c (the field and coefficients of
    tests/test_gpu_mg_accel.py's refresh test): the apply is a freshly built preconditioner's of the same form."""
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
    pc = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics, form=form, **inner)
    v = _cuda(np.random.default_rng(n).standard_normal(pc.shape[0]))
    before = pc.apply(v).clone()
    bp.update_theta_tables(*new_tabs)
    bp.eta_n = 1.0e4
    bp.refill(A, F, D, G, c=4.0, d_u=-1.0)
    pc.refresh()
    bp2 = mp.MultiphaseBlockPreconditioner(n, 1.0, 1.0e4, 1.0)
    bp2.set_theta_tables(*new_tabs)
    _, _, F2, D2, G2 = bp2.get_big_A_matrix(c=4.0, d_u=-1.0)
    fresh = mp.ApproxSchurPreconditioner(F2, D2, G2, numerics=numerics, form=form, **inner)
    assert pc.form == fresh.form == form and pc._plan.form == fresh._plan.form
    got = pc.apply(v)
    assert torch.equal(got, fresh.apply(v)) and not torch.equal(got, before)


# ------------------------------------------------------------------------------------ 7. refusals, nothing launched
def test_refusals_before_any_launch():
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    (A, F, D, G), _ = _system(16)
    with pytest.raises(ValueError, match="full.*upper.*lower.*diagonal"):
        mp.ApproxSchurPreconditioner(F, D, G, form="bogus")
    pc = mp.ApproxSchurPreconditioner(F, D, G, form="upper")
    v = _cuda(np.ones(pc.shape[0]))
    out = torch.full_like(v, float("nan"))
    # an unknown form
    pc._plan.form = 7
    try:
        with pytest.raises(_lib.MpbpError, match="form"):
            pc.apply(v, out)
    finally:
        pc._plan.form = _lib.FORM_UPPER
    # a row partition's plan (halo set) with a form other than full: refused, the callback never called
    called = []
    halo = _lib.HALO_FN(lambda *a: called.append("halo"))
    pc._plan.halo = halo
    try:
        for form in (_lib.FORM_UPPER, _lib.FORM_LOWER, _lib.FORM_DIAGONAL):
            pc._plan.form = form
            with pytest.raises(_lib.MpbpError, match="one-GPU"):
                pc.apply(v, out)
    finally:
        pc._plan.halo, pc._plan.form = _lib.HALO_FN(), _lib.FORM_UPPER
    torch.cuda.synchronize()
    assert not called
    assert bool(torch.isnan(out).all())     # nothing was written
    assert bool(torch.isfinite(pc.apply(v, out)).all())


# ------------------------------------------------------------------------------------ 8. solves
@pytest.mark.parametrize("eta_n", [100.0, 1.0e4])
@pytest.mark.parametrize("n", [16, 32])
def test_fgmres_converges_with_every_form(n, eta_n):
    """mpb.fgmres on the manufactured problem, exact numerics, mg:4 / mg:2, tol 1e-8, maxiter 150 (solve.py:285's own):
    every form converges to a true relative residual <= 1e-7.  (Dense CPU runs with exact inner solves needed at most
    30 iterations at these parameters; the counts are printed, no bar is put on them.)"""
    mp = _mp()
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    _, b = mp.manufactured_problem(n, xi=1.0, etan=eta_n, etas=1.0)
    bd = _cuda(b)
    nb = float(torch.linalg.vector_norm(bd))
    products, counts = (), {}
    for form in mp.FORMS:
        pc = mp.ApproxSchurPreconditioner(F, D, G, *products, inner_F=mp.InnerSolver("mg", 4),
                                          inner_P=mp.InnerSolver("mg", 2), form=form)
        products = (pc.GtG, pc.GtFG)
        hist = []
        x, info = mp.fgmres(A, bd, M=pc, tol=1e-8, maxiter=150, residuals=hist)
        res = float(torch.linalg.vector_norm(bd - A.matvec(x))) / nb
        counts[form] = len(hist) - 1
        assert info == 0 and res <= 1e-7, (form, info, res, counts)
    print(f"fgmres iterations n={n} eta_n={eta_n:g} mg:4/mg:2 exact: {counts}")


def test_solve_helper_passes_the_form_through():
    mp = _mp()
    n = 16
    u, b = mp.manufactured_problem(n, xi=1.0, etan=100.0, etas=1.0)
    kw = dict(inner_F=mp.InnerSolver("mg", 4), inner_P=mp.InnerSolver("mg", 2), verbose=False)
    _, info_u, hist_u = mp.solve_with_approx_schur_pc(n, 1.0, 100.0, 1.0, 1.0, -1.0, b, u, form="upper", **kw)
    _, info_f, hist_f = mp.solve_with_approx_schur_pc(n, 1.0, 100.0, 1.0, 1.0, -1.0, b, u, **kw)
    assert info_u == 0 and info_f == 0 and list(hist_u) != list(hist_f)
    with pytest.raises(ValueError):
        mp.solve_with_approx_schur_pc(n, 1.0, 100.0, 1.0, 1.0, -1.0, b, u, form="bogus", **kw)
