"""The phase-coupled multigrid smoother (Multigrid(smoother="coupled"), InnerSolver("mg", k, smoother="coupled")) on the
GPU.  Exact numerics are compared bit for bit against tests/coupled_smoother_restatement.py: the tables and bounds of
every smoothed level, mpbp_cpl_update in each of its forms, the standalone solve, the Schur apply with a coupled
inner_F; then fast against exact at the project's conditioning-floor rule, refresh, graph capture, the contraction at
large drag and the refusals."""
import functools

import numpy as np
import pytest

import block_forms_restatement as bf
import coupled_smoother_restatement as cr
from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_APPLY = 1e-12   # a fast apply is held to max(TOL_APPLY, 4 x the one-ulp floor), as tests/test_gpu_block_forms.py
# (xi, eta_n, eta_s); c = 1, d_u = -1 throughout
UNIT, DRAG, MIXED = (1.0, 100.0, 1.0), (1.0e6, 1.0, 1.0), (1.0e4, 1.0, 1.0e-4)
PRMS = {"unit": UNIT, "drag": DRAG, "mixed": MIXED}


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
    tabs = theta_tables(n)
    return tabs, StokesSystem(n, *prm, 1.0, -1.0, tables=tabs)


def _system(n, prm=UNIT):
    mp = _mp()
    tabs, S = _oracle_system(n, prm)
    bp = mp.MultiphaseBlockPreconditioner(n, *prm)
    bp.set_theta_tables(*tabs)
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    return (A, F, D, G), S


@functools.lru_cache(maxsize=None)
def _hierarchy(n, prm, coarsest, any_size=False):
    """The restatement's hierarchy, tables and intervals of F (built once per grid; the cycle's shape is set per use)."""
    _, S = _oracle_system(n, prm)
    return (cr.CoupledMgAnyOracle if any_size else cr.CoupledMgOracle)(S.F, n, coarsest=coarsest)


def _oracle_of(mg, prm):
    """The restatement of a coupled mg.Multigrid: the shared hierarchy with this one's cycle and coarse inverse, after
    checking that the GPU's tables and intervals are the restatement's bits."""
    import copy
    import scipy.sparse as sp
    ora = copy.copy(_hierarchy(mg.n, prm, mg.coarsest, mg.coarsen == "any"))
    ora.pre, ora.post, ora.cycles = mg.pre, mg.post, mg.cycles
    assert mg.sizes == [m for _, m in ora.ops] and mg.cpl[-1] is None
    for l, ((p, q), bnd) in enumerate(zip(ora.cpl, ora.bounds)):
        assert np.array_equal(_bits(mg.cpl[l][0]), _bits(p)) and np.array_equal(_bits(mg.cpl[l][1]), _bits(q)), l
        assert mg.bounds[l] == bnd, (l, mg.bounds[l], bnd)
    inv = np.asarray(mg.coarse_inv_host)
    m = inv.shape[0]
    ora.coarse_inv = inv
    ora._cinv = sp.csr_matrix((inv.reshape(-1), np.tile(np.arange(m), m), np.arange(0, m * m + 1, m)), shape=(m, m))
    return ora


# ------------------------------------------------------------------------------------------- 1. tables and bound
@pytest.mark.parametrize("prm", list(PRMS))
@pytest.mark.parametrize("n", [8, 16])
def test_tables_and_bound_bit_identical(n, prm):
    """F and every smoothed Galerkin level: cpl_p, cpl_q and lmax = ||B^-1 A||_inf are the restatement's bits."""
    mp = _mp()
    (A, F, D, G), S = _system(n, PRMS[prm])
    mg = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, smoother="coupled")
    assert mg.smoother == "coupled" and "smoother='coupled'" in repr(mg)
    ora = _oracle_of(mg, PRMS[prm])   # (asserts the tables and the intervals)
    assert len(ora.cpl) == mg.nlevels - 1 >= 1
    for l in range(mg.nlevels - 1):
        assert mg.bounds[l][0] == mg.bounds[l][1] / 4.0 and mg._levels[l].lmax == mg.bounds[l][1]
        assert mg._levels[l].cpl_p == mg.cpl[l][0].data_ptr() and mg._levels[l].cpl_q == mg.cpl[l][1].data_ptr()
    assert not mg._levels[mg.nlevels - 1].cpl_p
    point = mp.Multigrid(F, n, mp.FIELDS_VELOCITY)
    assert point.smoother == "point" and "smoother" not in repr(point) and point._mg.smoother == 0
    assert not point._levels[0].cpl_p and not point._levels[0].cpl_q


# ------------------------------------------------------------------------------------------- 2. mpbp_cpl_update
@pytest.mark.parametrize("aligned", [True, False], ids=["vec16", "scalar"])
@pytest.mark.parametrize("nrows", [64, 1296])
def test_cpl_update_every_form(nrows, aligned):
    """Random vectors, nrows = 64 and 1296 (no multiple of 256): the init, restart (d read as +0.0) and mid-solve forms,
    with and without sub, store_d 0 and 1 -- against the restatement, bit for bit.  aligned False: every vector starts
    8 bytes off a 16-byte boundary, which takes the element-wise kernel (same bits)."""
    from mp_block_preconditioners_amd._lib import check, lib, ptr, stream_handle
    rng = np.random.default_rng(nrows)
    off = 0 if aligned else 1

    def dev(x):   # a device copy at the wanted alignment
        buf = torch.empty(nrows + 2, dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + nrows]
        v.copy_(torch.from_numpy(x))
        return v
    p, q, r, x, d0, sub = (rng.standard_normal(nrows) for _ in range(6))
    p_d, q_d, r_d, x_d, sub_d = (dev(a) for a in (p, q, r, x, sub))   # (kept alive for every launch below)
    c1, c2 = 0.37, 1.21
    for form in ("init", "restart", "mid"):
        for use_sub in (False, True):
            for store_d in (0, 1):
                d_h = d0.copy()
                want = cr.update(p, q, r, None if form == "init" else x, c1, c2, d_h, sub if use_sub else None,
                                 dzero=form == "restart", store_d=bool(store_d))
                d_d, out = dev(d0), dev(np.full(nrows, np.nan))
                check(lib().mpbp_cpl_update(nrows, ptr(p_d), ptr(q_d), ptr(r_d), None if form == "init" else ptr(x_d),
                                            c1, c2, ptr(d_d), 1 if form == "restart" else 0,
                                            ptr(sub_d) if use_sub else None, ptr(out), store_d, stream_handle()))
                torch.cuda.synchronize()
                assert np.array_equal(_bits(out), _bits(want)), (form, use_sub, store_d)
                assert np.array_equal(_bits(d_d), _bits(d_h)), (form, use_sub, store_d)   # (store_d 0: untouched)
    with pytest.raises(Exception, match="multiple of 4"):
        check(lib().mpbp_cpl_update(6, ptr(p_d), ptr(q_d), ptr(r_d), None, c1, c2, ptr(d_d), 0, None, ptr(out), 1,
                                    stream_handle()))


# ------------------------------------------------------------------------------------------- 3. the standalone solve
def _standalone(n, prm, **kw):
    mp = _mp()
    (A, F, D, G), S = _system(n, PRMS[prm])
    mg = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, smoother="coupled", **kw)
    ora = _oracle_of(mg, PRMS[prm])
    rng = np.random.default_rng(n + mg.pre + 10 * mg.cycles)
    b, sub = rng.standard_normal(4 * n * n), rng.standard_normal(4 * n * n)
    return mg, ora, b, sub


@pytest.mark.parametrize("sell", [True, False], ids=["sell", "csr"])
@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("pre,post", [(2, 2), (1, 3)])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_standalone_solve_bit_identical(n, pre, post, cycles, sell):
    """Multigrid(F, n, FIELDS_VELOCITY, smoother="coupled").solve against the restated cycle, with and without sub (the
    zero start, the restart after the prolongation and of the second cycle, the last sweep's sub - x)."""
    prm = "drag" if n == 32 else "unit"
    mg, ora, b, sub = _standalone(n, prm, pre=pre, post=post, cycles=cycles, sell=sell)
    assert np.array_equal(_bits(mg.solve(_cuda(b))), _bits(ora.solve(b)))
    assert np.array_equal(_bits(mg.solve(_cuda(b), sub=_cuda(sub))), _bits(ora.solve(b, sub)))


@pytest.mark.parametrize("group_rows", [65536, 0], ids=["grp", "nogrp"])
def test_standalone_solve_other_level_kernels(group_rows):
    """The coarse levels off the grouped kernel (SELL rows; no k_grp_rr): the same bits."""
    mg, ora, b, sub = _standalone(32, "mixed", kernel_opts=dict(mg_group_rows=group_rows))
    assert np.array_equal(_bits(mg.solve(_cuda(b), sub=_cuda(sub))), _bits(ora.solve(b, sub)))


def test_standalone_solve_any_size():
    """coarsen="any" at n = 21 (levels 21, 10, 5): an odd level's pairs are still rows i and i + nrows / 2."""
    mg, ora, b, sub = _standalone(21, "drag", coarsen="any")
    assert mg.sizes == [21, 10, 5]
    assert np.array_equal(_bits(mg.solve(_cuda(b))), _bits(ora.solve(b)))
    assert np.array_equal(_bits(mg.solve(_cuda(b), sub=_cuda(sub))), _bits(ora.solve(b, sub)))


@pytest.mark.parametrize("K", [2, 3])
def test_standalone_solve_accelerated(K):
    """accel="chebyshev" with an explicit rho over the coupled cycle (B is symmetric, so V(2,2) stays symmetric)."""
    import mg_accel_restatement as ar
    rho = 0.2
    mg, ora, b, sub = _standalone(32, "drag", cycles=K, accel="chebyshev", rho=rho)
    assert "accel='chebyshev'" in repr(mg) and "smoother='coupled'" in repr(mg)
    want = ar.accel_solve(ar.oracle_vcycle(ora), b, K, rho, sub=sub)
    assert np.array_equal(_bits(mg.solve(_cuda(b), sub=_cuda(sub))), _bits(want))


# ------------------------------------------------------------------------------------------- 4. the Schur apply
def _point_oracle(mg, Mh):
    from oracle import mg_oracle as mo
    return mo.MgOracle(Mh, mg.n, mg.fields, mg.pre, mg.post, mg.cycles, bounds=mg.bounds,
                       coarse_inv=mg.coarse_inv_host, coarsest=mg.coarsest)


def _schur_case(n, prm, kF, forms=("full",), **kw):
    mp = _mp()
    (A, F, D, G), S = _system(n, PRMS[prm])
    v = np.random.default_rng(17 * n + kF).standard_normal(5 * n * n)
    products, solvers = (), None
    for form in forms:
        pc = mp.ApproxSchurPreconditioner(F, D, G, *products, inner_F=mp.InnerSolver("mg", kF, smoother="coupled"),
                                          inner_P=mp.InnerSolver("mg", 1), form=form, **kw)
        products = (pc.GtG, pc.GtFG)
        assert pc.mg_F.smoother == "coupled" and pc.mg_P.smoother == "point" and pc.inner_F.smoother == "coupled"
        if solvers is None:
            solvers = (bf.mg_solver(_oracle_of(pc.mg_F, PRMS[prm])), bf.mg_solver(_point_oracle(pc.mg_P, S.GtG)))
        want = bf.apply(form, S.F, S.D, S.G, S.GtG, S.GtFG, v, *solvers)
        got = pc.apply(_cuda(v))
        assert np.array_equal(_bits(got), _bits(want)), (form, rel_inf(got.cpu().numpy(), want))


@pytest.mark.parametrize("prm", ["unit", "drag"])
@pytest.mark.parametrize("kF", [1, 2])
@pytest.mark.parametrize("n", [16, 64, 96])
def test_schur_apply_bit_identical_to_the_restatement(n, kF, prm):
    """Exact numerics, a coupled inner_F (mg:1, mg:2) and inner_P mg:1, against the apply restated with the coupled F
    inverse plugged in.  n = 96 is where the point path takes every fused launch, so it tests their gating."""
    _schur_case(n, prm, kF)


def test_schur_apply_every_form():
    mp = _mp()
    _schur_case(16, "mixed", 1, forms=mp.FORMS)


# ------------------------------------------------------------------------------------------- 4b. one launch per sweep
@pytest.mark.parametrize("numerics", ["exact", "fast"])
@pytest.mark.parametrize("n,pre,post", [(5, 2, 2), (17, 2, 2), (64, 2, 2), (64, 1, 3), (257, 2, 2)])
def test_fused_level0_sweep_equals_the_two_launch_form(n, pre, post, numerics):
    """Level 0 the matrix-free F: each coupled sweep as one stencil launch with the cell-wise epilogue
    (Multigrid.set_coupled_fuse, mpbp_mg.cpl_fuse = 1, the default) against the residual launch + mpbp_cpl_update, bit
    for bit -- exact numerics (row<EDGE>'s sums either way) and fast (rows4's).  mg:2 in the full form reaches the zero
    start, the restarts (after the prolongation; the second cycle's pre-smoothing) and the second solve's sub - x.
    n = 5, 17: odd grids (coarsen="any"); n = 257: the marching kernel's second strip is one column wide."""
    mp = _mp()
    (A, F, D, G), _ = _system(n, DRAG)
    pc = mp.ApproxSchurPreconditioner(
        F, D, G, inner_F=mp.InnerSolver("mg", 2, pre=pre, post=post, smoother="coupled", coarsen="any"),
        inner_P=mp.InnerSolver("chebyshev", 3), numerics=numerics)
    assert pc.f_stencil is not None and pc.mg_F.cpl_fuse and pc.mg_F._mg.cpl_fuse == 1
    v = _cuda(np.random.default_rng(n).standard_normal(pc.shape[0]))
    fused = pc.apply(v).clone()
    pc.mg_F.set_coupled_fuse(False)
    assert pc.mg_F._mg.cpl_fuse == 0
    apart = pc.apply(v).clone()
    assert bool(torch.isfinite(fused).all()) and torch.equal(fused, apart), float((fused - apart).abs().max())
    for opts in (dict(f_direct=1),) if numerics == "fast" else ():   # the tolerance-mode rows on the direct kernel
        pc.set_kernel_opts(**opts)
        pc.mg_F.set_coupled_fuse(True)
        assert torch.equal(pc.apply(v), apart), opts


# ------------------------------------------------------------------------------------------- 5. fast numerics
@pytest.mark.parametrize("prm", ["unit", "drag"])
@pytest.mark.parametrize("n", [64, 96])
def test_fast_apply_at_the_conditioning_floor(n, prm):
    """Fast numerics against the exact GPU apply (section 4's bits), coupled inner_F mg:1, inner_P mg:1: within
    max(1e-12, 4 x floor), the floor being the exact apply's response to a one-ulp change of the input
    (tests/test_gpu_block_forms.py's rule).  Measured values: profiles/coupled_smoother_measured.txt."""
    mp = _mp()
    (A, F, D, G), _ = _system(n, PRMS[prm])
    kw = dict(inner_F=mp.InnerSolver("mg", 1, smoother="coupled"), inner_P=mp.InnerSolver("mg", 1))
    rng = np.random.default_rng(7 * n)
    v = rng.standard_normal(5 * n * n)
    v_ulp = v * (1.0 + np.where(rng.random(v.size) < 0.5, -1.0, 1.0) * 2.0 ** -52)
    fast = mp.ApproxSchurPreconditioner(F, D, G, numerics="fast", **kw)
    exact = mp.ApproxSchurPreconditioner(F, D, G, fast.GtG, fast.GtFG, **kw)
    ref = exact.apply(_cuda(v)).cpu().numpy()
    floor = rel_inf(exact.apply(_cuda(v_ulp)).cpu().numpy(), ref)
    err = rel_inf(fast.apply(_cuda(v)).cpu().numpy(), ref)
    print(f"coupled fast vs exact: n={n} {prm}: err {err:.3e}, one-ulp floor {floor:.3e}, "
          f"bound {max(TOL_APPLY, 4.0 * floor):.3e}")
    assert floor > 0.0
    assert err <= max(TOL_APPLY, 4.0 * floor), (err, floor)


# ------------------------------------------------------------------------------------------- 6. refresh
def test_refresh_matches_a_fresh_preconditioner():
    """update_theta_tables + refill with changed thn, c and d_u, then refresh: the tables and intervals are recomputed in
    place (same addresses) and the apply is a freshly built preconditioner's, bit for bit (n = 32)."""
    mp = _mp()
    from oracle.stokes_oracle import theta_tables
    n = 32
    inner = dict(inner_F=mp.InnerSolver("mg", 2, smoother="coupled"), inner_P=mp.InnerSolver("mg", 1))
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * x) * np.sin(4 * np.pi * y)
    new_tabs = (f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx))
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0e4, 1.0, 1.0)
    bp.set_theta_tables(*theta_tables(n))
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    pc = mp.ApproxSchurPreconditioner(F, D, G, **inner)
    v = _cuda(np.random.default_rng(n).standard_normal(pc.shape[0]))
    before = pc.apply(v).clone()
    where = [(t[0].data_ptr(), t[1].data_ptr()) for t in pc.mg_F.cpl if t is not None]
    bp.update_theta_tables(*new_tabs)
    bp.refill(A, F, D, G, c=4.0, d_u=-1.7)
    pc.refresh()
    bp2 = mp.MultiphaseBlockPreconditioner(n, 1.0e4, 1.0, 1.0)
    bp2.set_theta_tables(*new_tabs)
    _, _, F2, D2, G2 = bp2.get_big_A_matrix(c=4.0, d_u=-1.7)
    fresh = mp.ApproxSchurPreconditioner(F2, D2, G2, **inner)
    assert where == [(t[0].data_ptr(), t[1].data_ptr()) for t in pc.mg_F.cpl if t is not None]
    for l, t in enumerate(pc.mg_F.cpl):
        if t is not None:
            assert torch.equal(t[0], fresh.mg_F.cpl[l][0]) and torch.equal(t[1], fresh.mg_F.cpl[l][1]), l
    assert pc.mg_F.bounds == fresh.mg_F.bounds
    got = pc.apply(v)
    assert torch.equal(got, fresh.apply(v)) and not torch.equal(got, before)


# ------------------------------------------------------------------------------------------- 7. graph capture
@pytest.mark.parametrize("numerics", ["exact", "fast"])
def test_captured_apply_equals_eager(numerics):
    mp = _mp()
    n = 64
    (A, F, D, G), _ = _system(n, DRAG)
    pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("mg", 2, smoother="coupled"),
                                      inner_P=mp.InnerSolver("mg", 1), numerics=numerics)
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


# ------------------------------------------------------------------------------------------- 8. contraction
def test_contraction_at_large_drag():
    """Multigrid.contraction(steps=8)[-1] at n = 64, (xi, eta_n, eta_s) = (1e6, 100, 1): coupled < 0.3 and at most half
    of point.  The restatement gives 0.142 and 0.665 on the CPU (the same cycle, V(2,2), ratio 4, coarsest 8)."""
    mp = _mp()
    n = 64
    (A, F, D, G), _ = _system(n, (1.0e6, 100.0, 1.0))
    coupled = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, smoother="coupled").contraction(steps=8)[-1]
    point = mp.Multigrid(F, n, mp.FIELDS_VELOCITY).contraction(steps=8)[-1]
    print(f"contraction n={n} xi=1e6 eta 100/1, 8 steps: coupled {coupled:.4f}, point {point:.4f}")
    assert coupled < 0.3 and coupled <= 0.5 * point, (coupled, point)


# ------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd import distributed as dist
    n = 16
    (A, F, D, G), _ = _system(n)
    coupled = mp.InnerSolver("mg", 1, smoother="coupled")
    with pytest.raises(ValueError, match="pressure hierarchy has one field"):
        mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("mg", 1), inner_P=coupled)
    for kind in ("chebyshev", "jacobi"):
        with pytest.raises(ValueError, match="kind must be 'mg'"):
            mp.InnerSolver(kind, 4, smoother="coupled")
    with pytest.raises(ValueError, match="point.*coupled"):
        mp.InnerSolver("mg", 1, smoother="block")
    with pytest.raises(ValueError, match="point.*coupled"):
        mp.Multigrid(F, n, mp.FIELDS_VELOCITY, smoother="pair")
    GtG, _ = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)
    with pytest.raises(ValueError, match="four velocity fields"):
        mp.Multigrid(GtG, n, mp.FIELDS_PRESSURE, smoother="coupled")
    # the distributed classes: refused on the arguments alone, before any collective
    with pytest.raises(ValueError, match="one GPU only"):
        dist._check_setup_args(coupled, mp.InnerSolver("mg", 1), "auto", "auto", "auto", "auto", "sell", "exact")
    with pytest.raises(ValueError, match="one GPU only"):
        dist.DistributedSchurPreconditioner(n, 1.0, 100.0, 1.0, inner_F=coupled, inner_P=mp.InnerSolver("mg", 1))
    whole = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, smoother="coupled")
    with pytest.raises(ValueError, match="one GPU only"):
        dist.PartitionedMultigrid(whole, None, 4)
    # a stored zero on the diagonal: the block's determinant is -k k' <= 0; the error names the row, nothing is built
    Fh = F.to_scipy().tocsr()
    Fh.sort_indices()
    row = 5
    e = Fh.indptr[row] + int(np.flatnonzero(Fh.indices[Fh.indptr[row]:Fh.indptr[row + 1]] == row)[0])
    Fh.data[e] = 0.0
    Fz = mp.DeviceCSR.from_scipy(Fh)   # (from_scipy keeps stored zeros)
    with pytest.raises(_lib.MpbpError, match=r"first: row 5\)"):
        mp.Multigrid(Fz, n, mp.FIELDS_VELOCITY, smoother="coupled")
    # the C side: a coupled hierarchy without its tables, or under a row partition, is MPBP_ERR_ARG before any launch
    b = _cuda(np.ones(4 * n * n))
    out = torch.full_like(b, float("nan"))
    saved = whole._levels[0].cpl_p
    whole._levels[0].cpl_p = None
    try:
        with pytest.raises(_lib.MpbpError, match="cpl_p and cpl_q"):
            whole.solve(b, out=out)
    finally:
        whole._levels[0].cpl_p = saved
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert bool(torch.isfinite(whole.solve(b, out=out)).all())
