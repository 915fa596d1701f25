"""The fused tile kernels with general coefficients, on the reference's and on random thn tables, at their smallest grids.

The other files run these kernels only with xi = c = eta_s = d_p = 1, d_u = -1 on the reference's smooth thn, where
FStencilFast's -d_u xi, c face and d_u eta_s idx2 are exactly 1, face and -idx2 and PGDev::unit selects the specialised
Gt_G entries: a dropped, doubled or swapped coefficient in a fused kernel's cached per-cell terms changes no bit there.
Here every launch form runs off those values, bit for bit against the per-sweep launches it replaces and, for the fast
rows, against the oracle.

Coefficient sets (xi, eta_n, eta_s, c, d_u, d_p):
  general  (2.5, 3, 0.6, 0.7, -1.5, 2.5)   no factor is +-1 or a power of two; PGDev::unit off
  c0       (1, 1, 1, 0, -1, -0.75)         the eta_n == 1 identity instance, zero identity weight, negative d_p
  stiff    (1, 1e4, 1, 1, -1, 1)           BASELINE configs[3]
thn fields: "ref" (oracle.stokes_oracle.theta_tables) and "random" (three independent uniform(0.2, 0.8) tables,
default_rng(1000 + n): test_gpu_refresh._tables' random field).

Kernels, their gates (csrc/: ftile_ok in f_tile.inc, fsolve_ok in f_solve_w.inc, gtg_fused_ok in schur_inner.inc,
fpre_ok and gpre_ok in mg_solve.inc, gal_fused_ok and gal_pro_ok in schur_ops.inc) and the sizes that take them here:
  k_fsolve / k_fsolve_w   fsolve_ok: 3 updates n >= 70 (FsTile<2>::TW), 4 updates n >= 72 (FsTile<3>::TW); needs f_pair
                          -> kf = 3, 4 at n = 72, 76, 100, both tile forms (f_solve_tile 0: 64 x 8, 1: 32 x 16)
  k_ftile                 ftile_ok: n >= kFTW + kFTH + 4 = 76 -> n = 76, 100 (x0 + sweep 1 for every kf; the last pair
                          for kf = 4, 5 with f_pair); n = 72 stays on the marching kernels
  k_march2                f_pair, any n: the last two sweeps of kf >= 4 (f_tile off, or n = 72)
  direct F rows           f_direct, any n
  k_gtg_solve             gtg_fused_ok: n >= kGTW + kGTH + 2 (sweeps - 1) = 72 + 2 (kp - 1): 74, 78, 82 for kp = 2, 4, 6
                          (one bound for the 64 x 8 and the 32 x 16 tile) -> n = 82 (kp = 6's minimum), 100
  k_fpre                  fpre_ok: even n >= 72 -> n = 80, 96, 100
  k_gal1 / k_gal1p        gal_fused_ok: even n >= 2 kG1CW = 72 -> n = 80, 96, 100
  k_gtg_level0            gpre_ok: even n >= kGTW + kGTH + 6 = 78 -> n = 80, 96, 100
  k_gal1<PRO> / k_gal1p<PRO>  gal_pro_ok: n % 4 == 0, n / 4 >= kG1QW = 20, i.e. n >= 80, three levels -> n = 80, 96, 100
  k_grp_rr                the grouped small levels l >= 1 with a coarser level below: n = 80, 96 (five levels with
                          coarsest = 8; 100 coarsens to the odd 25: three levels)
100 is no multiple of the 64 x 8, 32 x 16 or coarse 32 x 4 / 16 x 8 tiles; 72 and 76 leave partial tiles too.

The multigrid section leaves c0 out: with c = 0 F is singular (constant velocities of both phases), and the coarsest
pseudo-inverse's cut-off (mg.COARSE_RCOND) was chosen from the spectra at c = 1.

Bars.  Bit equality wherever a launch form performs the per-sweep launches' operations.  Fast apply against
oracle/schur_oracle.py: north_star's 1e-12 relative inf-norm (TOL_APPLY of test_gpu_fast.py); the oracle apply's own
response to a one-ulp relative perturbation of every input entry is <= 2.7e-15 for these sets, fields and sizes, so the
reference sits ~400x inside the bar.  Multigrid fast apply against oracle/mg_oracle.py: max(1e-12, 4 x floor), floor =
the exact apply's response to one ulp per input entry, measured in the test (the rule of test_gpu_mg_1024.py); the
oracle's own floor for mg:1 / mg:1, coarsest 8 on these cases is 2.7e-14 .. 1.2e-13, so 1e-12 binds.  Measured values:
profiles/fused_params_measured.txt."""
import ctypes

import numpy as np
import pytest

from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_APPLY = 1e-12   # north_star: fp64 residuals within 1e-12 relative inf-norm

COEFFS = {"general": (2.5, 3.0, 0.6, 0.7, -1.5, 2.5),
          "c0": (1.0, 1.0, 1.0, 0.0, -1.0, -0.75),
          "stiff": (1.0, 1.0e4, 1.0, 1.0, -1.0, 1.0)}
FIELDS = ("ref", "random")
MG_COEFFS = ("general", "stiff")   # (c0: F singular, see the module docstring)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(oracle_built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for cache in (_TABLES, _SYSTEMS, _MG_PCS):   # (the n = 100 hierarchies hold 2500 x 2500 dense inverses)
        cache.clear()
    torch.cuda.empty_cache()


def _mp():
    import mp_block_preconditioners_amd as mp
    return mp


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


# ------------------------------------------------------------------------------------------------ shared inputs
_TABLES, _SYSTEMS, _MG_PCS = {}, {}, {}


def _tables(n, field):
    if (n, field) not in _TABLES:
        if field == "ref":
            from oracle.stokes_oracle import theta_tables
            tabs = theta_tables(n)
        else:
            rng = np.random.default_rng(1000 + n)
            tabs = tuple(rng.uniform(0.2, 0.8, n * n) for _ in range(3))
        _TABLES[n, field] = tuple(np.ascontiguousarray(t, dtype=np.float64) for t in tabs)
    return _TABLES[n, field]


def _oracle_system(n, coef, field):
    """oracle.stokes_oracle.StokesSystem of the case, built once (about 4 s of one host core at n = 100)."""
    key = (n, coef, field)
    if key not in _SYSTEMS:
        from oracle.stokes_oracle import StokesSystem
        xi, eta_n, eta_s, c, d_u, d_p = COEFFS[coef]
        _SYSTEMS[key] = StokesSystem(n, xi, eta_n, eta_s, c, d_u, d_p, tables=_tables(n, field))
    return _SYSTEMS[key]


def _operators(n, coef, field):
    xi, eta_n, eta_s, c, d_u, d_p = COEFFS[coef]
    bp = _mp().MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*_tables(n, field))
    _, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u, d_p=d_p)
    return F, D, G


def _input(pc, seed):
    return np.random.default_rng(seed).standard_normal(pc.shape[0])


def _replay(pc, v):
    out = torch.zeros_like(v)
    g = pc.capture(v, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    return out


def _same(got, ref, what):
    assert torch.equal(got, ref), (what, float((got - ref).abs().max()))


def _one_ulp(v, seed):
    """v with every entry moved by one ulp (relative 2^-52), seeded signs."""
    sign = np.where(np.random.default_rng(seed).random(v.size) < 0.5, -1.0, 1.0)
    return v * (1.0 + sign * 2.0 ** -52)


# ---------------------------------------------------------------------------- 1. fast F launch forms
# Every form names all four options: k_fsolve and the tile pair are taken only with f_pair on (f_pair_ok), so the
# forms switch on what the kernel they are about needs.
F_BASE = dict(f_solve=0, f_tile=0, f_pair=0, f_direct=0)           # the per-sweep marching launches
F_FORMS = [("f_direct", dict(F_BASE, f_direct=1)),                  # the per-sweep direct kernel
           ("f_pair", dict(F_BASE, f_pair=1)),                      # k_march2
           ("f_tile", dict(F_BASE, f_tile=1)),                      # k_ftile<INIT>, marching sweeps after it
           ("f_tile+f_pair", dict(F_BASE, f_tile=1, f_pair=1)),     # ... and the last pair on tiles
           ("f_solve 64x8", dict(F_BASE, f_tile=1, f_pair=1, f_solve=1, f_solve_tile=0)),
           ("f_solve 32x16", dict(F_BASE, f_tile=1, f_pair=1, f_solve=1, f_solve_tile=1))]   # (last: the defaults)


@pytest.mark.parametrize("kf", [2, 3, 4, 5])
@pytest.mark.parametrize("n", [72, 76, 100])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("coef", list(COEFFS))
def test_fast_f_launch_forms(coef, field, n, kf):
    """A fast F Chebyshev solve of kf updates in each launch form -- direct rows, k_march2, k_ftile, k_fsolve on 64 x 8
    tiles, k_fsolve_w on 32 x 16 tiles -- with G x_p recomputed inside the second solve (fuse_g) and launched apart:
    bit-identical to the per-sweep marching launches, the default form's graph replay bit-identical to its eager apply,
    and the marching apply within 1e-12 of oracle/schur_oracle.py's on the same operators and interval."""
    mp = _mp()
    from oracle.schur_oracle import Inner, approx_schur_apply
    F, D, G = _operators(n, coef, field)
    kw = dict(inner_F=mp.InnerSolver("chebyshev", kf), inner_P=mp.InnerSolver("chebyshev", 4), numerics="fast")
    fused = mp.ApproxSchurPreconditioner(F, D, G, fuse_g=True, **kw)
    apart = mp.ApproxSchurPreconditioner(F, D, G, fused.GtG, fused.GtFG, fuse_g=False, **kw)
    assert fused.fuse_g and not apart.fuse_g
    assert fused.f_stencil is not None and fused.pg_stencil is not None
    vh = _input(fused, 10 * n + kf)
    v = _cuda(vh)
    base = None
    for name, pc in (("fuse_g", fused), ("G apart", apart)):
        pc.set_kernel_opts(**F_BASE)
        ref = pc.apply(v).clone()
        if base is None:
            base = ref
        _same(ref, base, name)           # G x_p recomputed == G launched, W streamed
        for form, opts in F_FORMS:
            pc.set_kernel_opts(**opts)
            _same(pc.apply(v), ref, (name, form))
        _same(_replay(pc, v), ref, (name, "replay"))
    S = _oracle_system(n, coef, field)
    want = approx_schur_apply(S.F, S.D, S.G, S.GtG, S.GtFG, vh,
                              Inner("chebyshev", kf, fused.inner_F.lmin, fused.inner_F.lmax),
                              Inner("chebyshev", 4, fused.inner_P.lmin, fused.inner_P.lmax))
    err = rel_inf(base.cpu().numpy(), want)
    print(f"fast F forms {coef} {field} n={n} kf={kf}: marching vs oracle {err:.3e}")
    assert 0.0 < err <= TOL_APPLY, err   # (> 0: the fast rows really ran)


# ---------------------------------------------------------------------------- 2. fused Gt_G solve
@pytest.mark.parametrize("numerics", ["exact", "fast"])
@pytest.mark.parametrize("kp", [2, 4, 6])
@pytest.mark.parametrize("n", [82, 100])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("coef", list(COEFFS))
def test_fused_gtg_solve_forms(coef, field, n, kp, numerics):
    """k_gtg_solve off PGDev::unit (d_p = 2.5, -0.75) and on it (stiff): both tile forms (gtg_solve_tile 0: 64 x 8, 1:
    32 x 16), 256- and 512-lane workgroups, with the first solve building rhs = D Finv_v + v_p itself (gtg_drhs) or
    reading the D launch's -- each bit-identical to the per-sweep Gt_G launches.  n = 82 is the gate's minimum for
    kp = 6 (72 + 2 (kp - 1), the same for both tiles)."""
    mp = _mp()
    assert n >= 72 + 2 * (kp - 1)        # gtg_fused_ok: every case here takes the fused solve
    F, D, G = _operators(n, coef, field)
    pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("chebyshev", 4),
                                      inner_P=mp.InnerSolver("chebyshev", kp), numerics=numerics)
    assert pc.pg_stencil is not None
    v = _cuda(_input(pc, 10 * n + kp))
    pc.set_kernel_opts(gtg_fused=0)
    ref = pc.apply(v).clone()
    assert bool(torch.isfinite(ref).all())
    for tile in (0, 1):
        for tpb in (256, 512):
            for drhs in (0, 1):
                pc.set_kernel_opts(gtg_fused=1, gtg_solve_tile=tile, gtg_tpb=tpb, gtg_drhs=drhs)
                _same(pc.apply(v), ref, dict(tile=tile, tpb=tpb, drhs=drhs))


# ---------------------------------------------------------------------------- 3. multigrid fusions
def _mg_pc(coef, field, n, numerics, cycles):
    """The Schur preconditioner with mg:cycles / mg:cycles inner solves (coarsest 8), built once per case; tests put
    the kernel options they change back (_restored)."""
    key = (coef, field, n, numerics, cycles)
    if key not in _MG_PCS:
        mp = _mp()
        F, D, G = _operators(n, coef, field)
        _MG_PCS[key] = mp.ApproxSchurPreconditioner(F, D, G, numerics=numerics,
                                                    inner_F=mp.InnerSolver("mg", cycles, coarsest=8),
                                                    inner_P=mp.InnerSolver("mg", cycles, coarsest=8))
    pc = _MG_PCS[key]
    ko = pc.kernel_opts
    assert (ko.mg_fuse_l0, ko.mg_fuse_small, ko.f_tile, ko.mg_galerkin_mf, ko.mg_galerkin_mf_p) == (1, 1, 1, 2, 1)
    return pc


def _toggled(pc, v, **opts):
    """The apply with `opts` changed, the previous choices put back after it."""
    before = {k: getattr(pc.kernel_opts, k) for k in opts}
    pc.set_kernel_opts(**opts)
    try:
        return pc.apply(v).clone()
    finally:
        pc.set_kernel_opts(**before)


MG_CASES = [(c, f, n) for c in MG_COEFFS for f in FIELDS for n in (80, 96, 100)]
MG_IDS = [f"{c}-{f}-{n}" for c, f, n in MG_CASES]


@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("coef,field,n", MG_CASES, ids=MG_IDS)
def test_mg_fusions_equal_launches_fast(coef, field, n, cycles):
    """Fast numerics: the default multigrid apply (k_fpre, k_gtg_level0, k_gal1 / k_gal1p and their <PRO> ascents,
    k_grp_rr, the level-0 tile pair) is bit-identical to the apply with each fusion switched back alone -- mg_fuse_l0,
    mg_fuse_small, f_tile, and mg_galerkin_mf = 1 (level 1 as three launches) -- and to its graph replay."""
    pc = _mg_pc(coef, field, n, "fast", cycles)
    assert len(pc.mg_F.sizes) >= 3 and len(pc.mg_P.sizes) >= 3
    v = _cuda(_input(pc, 3 * n + cycles))
    ref = pc.apply(v).clone()
    assert bool(torch.isfinite(ref).all())
    for opts in (dict(mg_fuse_l0=0), dict(mg_fuse_small=0), dict(f_tile=0), dict(mg_galerkin_mf=1)):
        _same(_toggled(pc, v, **opts), ref, opts)
    _same(_replay(pc, v), ref, "replay")


@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("coef,field,n", MG_CASES, ids=MG_IDS)
def test_mg_fusions_equal_launches_exact(coef, field, n, cycles):
    """Exact numerics: k_gtg_level0 (the pressure hierarchy's level 0) and k_grp_rr on and off, bit for bit."""
    pc = _mg_pc(coef, field, n, "exact", cycles)
    v = _cuda(_input(pc, 3 * n + cycles))
    ref = pc.apply(v).clone()
    assert bool(torch.isfinite(ref).all())
    for opts in (dict(mg_fuse_l0=0), dict(mg_fuse_small=0)):
        _same(_toggled(pc, v, **opts), ref, opts)


@pytest.mark.parametrize("coef,field,n", MG_CASES, ids=MG_IDS)
def test_mg_matrix_free_level1_vs_stored(coef, field, n):
    """The fused level 1 (k_gal1 for F, k_gal1p for Gt_G) is really taken at these sizes -- mpbp_mg_level1_apply returns
    OK for both hierarchies and agrees with the stored Galerkin matrix -- and the apply with the stored level 1
    (mg_galerkin_mf = 0: both hierarchies; mg_galerkin_mf_p = 0: the pressure one) is another summation order of the
    same operator: within 1e-12 of the default, and not its bits."""
    from mp_block_preconditioners_amd._lib import VEC_PRESSURE, VEC_VELOCITY, check, lib, ptr, stream_handle
    pc = _mg_pc(coef, field, n, "fast", 1)
    v = _cuda(_input(pc, 3 * n + 1))
    ref = pc.apply(v).cpu().numpy()
    for opts in (dict(mg_galerkin_mf=0), dict(mg_galerkin_mf_p=0)):
        err = rel_inf(_toggled(pc, v, **opts).cpu().numpy(), ref)
        print(f"mg level 1 {coef} {field} n={n} {opts}: stored vs matrix-free {err:.3e}")
        assert 0.0 < err <= TOL_APPLY, (opts, err)
    gen = torch.Generator(device="cuda").manual_seed(n + 7)
    for kind, mg in ((VEC_VELOCITY, pc.mg_F), (VEC_PRESSURE, pc.mg_P)):
        M1 = mg.ops[1]
        x = torch.randn(M1.shape[0], dtype=torch.float64, device="cuda", generator=gen)
        y = torch.full_like(x, 7.0)
        check(lib().mpbp_mg_level1_apply(ctypes.byref(pc._plan), kind, 0, ptr(x), None, ptr(y), stream_handle()))
        e1 = rel_inf(y.cpu().numpy(), M1.matvec(x).cpu().numpy())
        print(f"mg level 1 {coef} {field} n={n} kind {kind}: fused product vs stored matrix {e1:.3e}")
        assert e1 <= TOL_APPLY, (kind, e1)


def _oracle_mg_apply(S, pc, v):
    """approx_schur_op (solve.py:257-277) with oracle/mg_oracle.py's V-cycles as both inner inverses on the oracle's
    own operators, with the GPU hierarchy's bounds and coarsest inverses (test_gpu_fast._oracle_mg_apply)."""
    from oracle import csr_oracle as co
    from oracle import mg_oracle as mo
    mF, mP = pc.mg_F, pc.mg_P
    oF = mo.MgOracle(S.F, mF.n, mF.fields, mF.pre, mF.post, mF.cycles, bounds=mF.bounds,
                     coarse_inv=mF.coarse_inv_host, coarsest=mF.coarsest)
    oP = mo.MgOracle(S.GtG, mP.n, mP.fields, mP.pre, mP.post, mP.cycles, bounds=mP.bounds,
                     coarse_inv=mP.coarse_inv_host, coarsest=mP.coarsest)
    assert [M.shape[0] for M, _ in oF.ops] == [M.shape[0] for M in mF.ops]
    nu = S.F.shape[0]
    Finv_v = oF.solve(v[:nu])
    x_a = oP.solve(co.spmv(S.D, Finv_v, v[nu:], mode=1))
    x_p = oP.solve(co.spmv(S.GtFG, x_a))
    return np.concatenate([oF.solve(co.spmv(S.G, x_p), sub=Finv_v), x_p])


@pytest.mark.parametrize("coef,field,n", MG_CASES, ids=MG_IDS)
def test_mg_fast_apply_vs_mg_oracle(coef, field, n):
    """The default fast mg:1 / mg:1 apply against oracle/mg_oracle.py inside schur_oracle's composition, held to
    max(1e-12, 4 x floor); floor: the exact apply of the input moved by one ulp per entry, against the exact apply.
    On a miss the fast components are switched back one at a time and each error is reported."""
    pc = _mg_pc(coef, field, n, "fast", 1)
    exact = _mg_pc(coef, field, n, "exact", 1)
    vh = _input(pc, 3 * n + 1)
    want = _oracle_mg_apply(_oracle_system(n, coef, field), pc, vh)
    ex = exact.apply(_cuda(vh)).cpu().numpy()
    floor = rel_inf(exact.apply(_cuda(_one_ulp(vh, n))).cpu().numpy(), ex)
    err = rel_inf(pc.apply(_cuda(vh)).cpu().numpy(), want)
    print(f"mg fast vs oracle {coef} {field} n={n}: err {err:.3e} floor {floor:.3e} "
          f"(exact vs oracle {rel_inf(ex, want):.3e})")
    assert floor > 0.0
    # the exact apply performs the oracle's operations in the oracle's order (tests/test_gpu_mg.py): its bits
    assert np.array_equal(ex.view(np.uint64), want.view(np.uint64)), rel_inf(ex, want)
    bar = max(TOL_APPLY, 4.0 * floor)
    if not err <= bar:
        back = {}
        for opts in (dict(mg_galerkin_mf=0), dict(mg_galerkin_mf_p=0), dict(q13_sym=0), dict(q13_mf=0),
                     dict(f_tile=0)):
            back[next(iter(opts))] = rel_inf(_toggled(pc, _cuda(vh), **opts).cpu().numpy(), want)
        print("  with one component switched back:", back)
    assert 0.0 < err <= bar, (err, floor)
