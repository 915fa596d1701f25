"""In-place refresh for a new volume-fraction field (a time step: same grid, same sparsity, new values).

"fresh" objects are built from scratch with the new tables and coefficients; "refreshed" ones are built with the
reference's thn (mpbp_stokes_theta) and c = 1, d_u = -1, then updated in place (update_theta_tables, refill,
refresh_products, Multigrid.refresh, ApproxSchurPreconditioner.refresh).  The refresh runs the builders' arithmetic in
the builders' order, so every comparison is bit equality (torch.equal): no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _mp():
    import mp_block_preconditioners_amd as mp
    return mp


def _tables(n, kind):
    """theta_1: the smooth field 0.5 + 0.3 cos(2 pi x) sin(4 pi y) at the three tables' points, or seeded random tables."""
    if kind == "random":
        rng = np.random.default_rng(1000 + n)
        return tuple(rng.uniform(0.2, 0.8, n * n) for _ in range(3))
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * x) * np.sin(4 * np.pi * y)
    return f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx)


# (tables, c, d_u, eta_n): the two fields, and one step that also changes the coefficients
STEPS = [("smooth", 1.0, -1.0, 100.0), ("random", 1.0, -1.0, 100.0), ("smooth", 4.0, -0.5, 1e4)]
# (tables, c, d_u, eta_n, xi, eta_s, d_p): every coefficient the steps above leave at 1 -- xi and eta_s (the fast F rows'
# -d_u xi and d_u eta_s idx2) and d_p (2.5 switches the Gt_G rows' d_p == 1 specialisation off)
STEP_ALL = ("random", 0.7, -1.5, 100.0, 2.5, 0.6, 2.5)


def _unpack(step):
    """(tables, c, d_u, eta_n, xi, eta_s, d_p) of a step; xi = eta_s = d_p = 1 where it does not name them."""
    return tuple(step) + (1.0, 1.0, 1.0)[len(step) - 4:]


def _fresh(n, step):
    kind, c, d_u, eta_n, xi, eta_s, d_p = _unpack(step)
    bp = _mp().MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    bp.set_theta_tables(*_tables(n, kind))
    A, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u, d_p=d_p)
    return bp, (A, F, D, G)


def _start(n):
    """theta_0 objects: the reference's thn, c = 1, d_u = -1."""
    bp = _mp().MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    return bp, (A, F, D, G)


def _step_to(bp, ops, step, n):
    kind, c, d_u, eta_n, xi, eta_s, d_p = _unpack(step)
    bp.update_theta_tables(*_tables(n, kind))
    bp.xi, bp.eta_n, bp.eta_s = xi, eta_n, eta_s
    bp.refill(*ops, c=c, d_u=d_u, d_p=d_p)


def _same_values(got, ref, what=""):
    assert torch.equal(got.row_ptr, ref.row_ptr) and torch.equal(got.col_idx, ref.col_idx), what
    assert torch.equal(got.val, ref.val), what


def _blank(ref):
    """ref's pattern with NaN values (a refill must write every entry)."""
    from mp_block_preconditioners_amd.csr import DeviceCSR
    return DeviceCSR(ref.row_ptr.clone(), ref.col_idx.clone(), torch.full_like(ref.val, float("nan")), ref.shape)


def _refill_pair(A, B, alpha, C):
    from mp_block_preconditioners_amd._lib import check, lib, stream_handle
    check(lib().mpbp_spgemm_refill(ctypes.byref(A.cstruct()), ctypes.byref(B.cstruct()), alpha,
                                   ctypes.byref(C.cstruct()), stream_handle()))


def _refill_triple(X, Y, Z, assoc, ai, ao, C):
    from mp_block_preconditioners_amd._lib import check, lib, stream_handle
    check(lib().mpbp_triple_refill(ctypes.byref(X.cstruct()), ctypes.byref(Y.cstruct()), ctypes.byref(Z.cstruct()),
                                   assoc, ai, ao, ctypes.byref(C.cstruct()), stream_handle()))


# ---------------------------------------------------------------------------------------------- 1. products
@pytest.fixture(scope="module")
def random_xyz():
    """Seeded X (40 x 30), Y (30 x 35), Z (35 x 64): empty rows in each, Z's row 5 full, and X Y's row 0 reaching it --
    so row 0 of X Y Z holds 64 entries, the widest a product row may be; columns are hit by many products."""
    from mp_block_preconditioners_amd.csr import DeviceCSR
    rng = np.random.default_rng(42)

    def rnd(m, k, density):
        M = sp.random(m, k, density=density, random_state=rng, data_rvs=rng.standard_normal, format="lil")
        return M
    X, Y, Z = rnd(40, 30, 0.12), rnd(30, 35, 0.12), rnd(35, 64, 0.08)
    for M, rows in ((X, (3, 17)), (Y, (4,)), (Z, (9,))):
        for r in rows:
            M[r, :] = 0.0
    X[0, 2], Y[2, 5] = 1.5, 0.7
    Z[5, :] = rng.standard_normal(64)
    mats = []
    for M in (X, Y, Z):
        M = sp.csr_matrix(M)
        M.eliminate_zeros()
        mats.append(DeviceCSR.from_scipy(M))
    return mats


def test_pair_refill_matches_spgemm(random_xyz):
    from mp_block_preconditioners_amd.csr import spgemm
    X, Y, Z = random_xyz
    for A, B, alpha in ((X, Y, -2.5), (Y, Z, 0.375), (X, Y, 1.0)):
        ref = spgemm(A, B, alpha)
        C = _blank(ref)
        _refill_pair(A, B, alpha, C)
        _same_values(C, ref)
    lens = np.diff(spgemm(Y, Z).row_ptr_host)
    assert lens.max() == 64 and lens.min() == 0      # the full row and an empty one were exercised


@pytest.mark.parametrize("assoc", ["left", "right"])
def test_triple_refill_matches_two_spgemms(random_xyz, assoc):
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.csr import spgemm
    X, Y, Z = random_xyz
    ai, ao = -1.75, 0.3
    if assoc == "left":
        inner = spgemm(X, Y, ai)
        ref = spgemm(inner, Z, ao)
    else:
        inner = spgemm(Y, Z, ai)
        ref = spgemm(X, inner, ao)
    lens = np.diff(ref.row_ptr_host)
    assert lens.max() == 64 and lens.min() == 0 and np.diff(inner.row_ptr_host).min() == 0
    C = _blank(ref)
    _refill_triple(X, Y, Z, _lib.ASSOC_LEFT if assoc == "left" else _lib.ASSOC_RIGHT, ai, ao, C)
    _same_values(C, ref)


def test_refill_error_paths(random_xyz):
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.csr import DeviceCSR, spgemm
    one = DeviceCSR.from_scipy(sp.csr_matrix(np.ones((1, 1))))
    wide = DeviceCSR.from_scipy(sp.csr_matrix(np.ones((1, 65))))
    tall = DeviceCSR.from_scipy(sp.csr_matrix(np.ones((65, 1))))
    # a 65-entry output row
    with pytest.raises(_lib.MpbpError, match="wider than 64"):
        _refill_pair(one, wide, 1.0, _blank(wide))
    with pytest.raises(_lib.MpbpError, match="wider than 64"):
        _refill_triple(one, one, wide, _lib.ASSOC_RIGHT, 1.0, 1.0, _blank(wide))
    # a 65-entry inner row (X Y) under a one-entry output row
    with pytest.raises(_lib.MpbpError, match="wider than 64"):
        _refill_triple(one, wide, tall, _lib.ASSOC_LEFT, 1.0, 1.0, _blank(one))
    # a pattern that lacks a column of the product
    X, Y, Z = random_xyz
    ref = spgemm(X, Y).to_scipy().tocoo()
    keep = np.ones(ref.nnz, dtype=bool)
    keep[ref.nnz // 2] = False
    lacking = DeviceCSR.from_scipy(sp.csr_matrix((ref.data[keep], (ref.row[keep], ref.col[keep])), shape=ref.shape))
    with pytest.raises(_lib.MpbpError, match="lack a column"):
        _refill_pair(X, Y, 1.0, lacking)
    full = spgemm(spgemm(X, Y), Z).to_scipy().tocoo()
    keep = np.ones(full.nnz, dtype=bool)
    keep[0] = False
    lacking = DeviceCSR.from_scipy(sp.csr_matrix((full.data[keep], (full.row[keep], full.col[keep])), shape=full.shape))
    for assoc in (_lib.ASSOC_LEFT, _lib.ASSOC_RIGHT):
        with pytest.raises(_lib.MpbpError, match="lack a column"):
            _refill_triple(X, Y, Z, assoc, 1.0, 1.0, lacking)
    # shapes
    with pytest.raises(_lib.MpbpError, match="shape mismatch"):
        _refill_pair(X, Z, 1.0, _blank(X))
    with pytest.raises(_lib.MpbpError, match="shape mismatch"):
        _refill_triple(X, Y, Z, _lib.ASSOC_LEFT, 1.0, 1.0, _blank(X))


@pytest.mark.parametrize("step", STEPS, ids=[s[0] + ("+coef" if s[1] != 1.0 else "") for s in STEPS])
def test_refresh_products_matches_commutator_products(step):
    mp = _mp()
    n = 16
    bp, ops = _start(n)
    GtG, GtFG = mp.MultiphaseBlockPreconditioner.commutator_products(*ops[1:])
    ptrs = (GtG.val.data_ptr(), GtFG.val.data_ptr())
    _step_to(bp, ops, step, n)
    mp.MultiphaseBlockPreconditioner.refresh_products(*ops[1:], GtG, GtFG)
    _, fops = _fresh(n, step)
    rG, rQ = mp.MultiphaseBlockPreconditioner.commutator_products(*fops[1:])
    _same_values(GtG, rG, "Gt_G")
    _same_values(GtFG, rQ, "Gt_F_G")
    assert ptrs == (GtG.val.data_ptr(), GtFG.val.data_ptr())


@pytest.mark.parametrize("fields", ["velocity", "pressure"])
def test_galerkin_level_matches_two_spgemms(fields):
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.csr import spgemm
    from mp_block_preconditioners_amd.mg import transfer
    n = 16
    _, (A, F, D, G) = _fresh(n, STEPS[1])
    if fields == "velocity":
        M, kinds = F, mp.FIELDS_VELOCITY
    else:
        M, kinds = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)[0], mp.FIELDS_PRESSURE
    P = transfer(n, kinds, _lib.MG_P, M.device)
    R = transfer(n, kinds, _lib.MG_R, M.device)
    ref = spgemm(R, spgemm(M, P))
    C = _blank(ref)
    _refill_triple(R, M, P, _lib.ASSOC_RIGHT, 1.0, 1.0, C)
    _same_values(C, ref)


# --------------------------------------------------------------------------------------------- 2. operators
@pytest.mark.parametrize("n", [3, 8, 32])
def test_refill_matches_fresh_assembly(n):
    bp, ops = _start(n)
    ptrs = [(M.row_ptr.data_ptr(), M.col_idx.data_ptr(), M.val.data_ptr()) for M in ops]
    cols = [M.col_idx.clone() for M in ops]
    tabs = [t.data_ptr() for t in bp.theta_tables()]
    for step in STEPS:
        _step_to(bp, ops, step, n)
        _, fops = _fresh(n, step)
        for name, M, ref, ci in zip("AFDG", ops, fops, cols):
            _same_values(M, ref, (name, step))
            assert torch.equal(M.col_idx, ci)
        assert ptrs == [(M.row_ptr.data_ptr(), M.col_idx.data_ptr(), M.val.data_ptr()) for M in ops]
        assert tabs == [t.data_ptr() for t in bp.theta_tables()]
    if n >= 3:   # the stencils' shared parameters follow (matrix-free F with the refilled coefficients == assembled F)
        x = torch.from_numpy(np.random.default_rng(n).standard_normal(ops[1].shape[1])).cuda()
        assert torch.equal(ops[1].stencil.matvec(x), ops[1].matvec(x))
    # another grid's operators are refused
    _, other = _start(n + 1)
    with pytest.raises(ValueError):
        bp.refill(*other, c=1.0, d_u=-1.0)


def test_update_theta_tables_creates_missing_tables():
    n = 8
    bp = _mp().MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    tabs = _tables(n, "smooth")
    bp.update_theta_tables(*tabs)
    for t, ref in zip(bp.theta_tables(), tabs):
        assert np.array_equal(t.cpu().numpy(), ref)


# ------------------------------------------------------------------------------ 3. standalone Multigrid.refresh
def _same_hierarchy(mg, ref):
    assert mg.sizes == ref.sizes and mg.nlevels == ref.nlevels
    assert mg.bounds == ref.bounds
    for l in range(mg.nlevels):
        _same_values(mg.ops[l], ref.ops[l], f"level {l}")
        assert torch.equal(mg.diags[l], ref.diags[l]), l
        assert (mg._levels[l].lmin, mg._levels[l].lmax) == (ref._levels[l].lmin, ref._levels[l].lmax) == ref.bounds[l]
        S, Sr = mg.sells[0][l], ref.sells[0][l]
        assert (S is None) == (Sr is None)
        if S is not None:
            assert torch.equal(S.val, Sr.val) and torch.equal(S.col, Sr.col) and torch.equal(S.row_len, Sr.row_len)
        V, Vr = mg.svls[l], ref.svls[l]
        assert (V is None) == (Vr is None)
        if V is not None:
            assert torch.equal(V.vals, Vr.vals)
    assert torch.equal(mg.coarse_inv.val, ref.coarse_inv.val)
    assert torch.equal(mg.coarse_dense, ref.coarse_dense)
    assert np.array_equal(mg.coarse_inv_host, ref.coarse_inv_host)


@pytest.mark.parametrize("fields,svl", [("velocity", "default"), ("pressure", "default"), ("velocity", 0)],
                         ids=["velocity", "pressure", "velocity-svl"])
def test_multigrid_refresh_matches_fresh_hierarchy(fields, svl):
    mp = _mp()
    n, step = 32, STEPS[2]
    kinds = mp.FIELDS_VELOCITY if fields == "velocity" else mp.FIELDS_PRESSURE

    def operator(ops):
        return ops[1] if fields == "velocity" else mp.MultiphaseBlockPreconditioner.commutator_products(*ops[1:])[0]
    bp, ops = _start(n)
    M = operator(ops)
    mg = mp.Multigrid(M, n, kinds, coarsest=4, cycles=2, svl_min_rows=svl)
    assert mg.sizes == [32, 16, 8, 4]
    if svl == 0:
        assert any(V is not None for V in mg.svls)
    _step_to(bp, ops, step, n)
    if fields == "pressure":
        _refill_pair(ops[2], ops[3], -1.0, M)
    mg.refresh()
    _, fops = _fresh(n, step)
    ref = mp.Multigrid(operator(fops), n, kinds, coarsest=4, cycles=2, svl_min_rows=svl)
    _same_hierarchy(mg, ref)
    b = torch.from_numpy(np.random.default_rng(3).standard_normal(M.shape[0])).cuda()
    assert torch.equal(mg.solve(b), ref.solve(b))


# ------------------------------------------------------------------------------------------ 4. preconditioner
def _inner(spec):
    kind, _, k = spec.partition(":")
    return _mp().InnerSolver(kind, int(k), coarsest=8)


def _pc(ops, inner, **kw):
    return _mp().ApproxSchurPreconditioner(*ops[1:], inner_F=_inner(inner[0]), inner_P=_inner(inner[1]), **kw)


PAIRS = [("chebyshev:4", "chebyshev:4"), ("mg:2", "mg:1"), ("jacobi:3", "chebyshev:4")]


def _same_with(pc, v, alt):
    """The refreshed preconditioner's apply is the same bits with the kernel options `alt` (the launches a fused kernel
    replaces: both read the refreshed state alike); the options are put back."""
    if not alt:
        return
    got = pc.apply(v).clone()
    before = {k: getattr(pc.kernel_opts, k) for k in alt}
    pc.set_kernel_opts(**alt)
    other = pc.apply(v).clone()
    pc.set_kernel_opts(**before)
    assert torch.equal(other, got), (alt, float((other - got).abs().max()))


def _back_to_start(bp, ops, theta0):
    bp.update_theta_tables(*theta0)
    bp.xi, bp.eta_n, bp.eta_s = 1.0, 100.0, 1.0
    bp.refill(*ops, c=1.0, d_u=-1.0)


def _refresh_walk(n, inner, alt=None, **kw):
    """theta_0 -> smooth field -> random tables with new coefficients -> theta_0, the apply against a fresh
    preconditioner's after each refresh, the original apply after the last; then a graph captured after the refreshes.
    alt: kernel options under which the refreshed apply must not change by a bit, checked after every refresh."""
    bp, ops = _start(n)
    theta0 = [t.clone() for t in bp.theta_tables()]
    pc = _pc(ops, inner, **kw)
    v = torch.from_numpy(np.random.default_rng(n).standard_normal(pc.shape[0])).cuda()
    first = pc.apply(v).clone()
    plan = id(pc._plan)
    assert pc.generation == 0
    for i, step in enumerate((STEPS[0], ("random",) + STEPS[2][1:])):
        _step_to(bp, ops, step, n)
        pc.refresh()
        assert pc.generation == i + 1
        _, fops = _fresh(n, step)
        ref = _pc(fops, inner, **kw)
        assert (pc.inner_F.lmin, pc.inner_F.lmax, pc.inner_P.lmin, pc.inner_P.lmax) == \
            (ref.inner_F.lmin, ref.inner_F.lmax, ref.inner_P.lmin, ref.inner_P.lmax)
        assert torch.equal(pc.apply(v), ref.apply(v)), step
        del ref, fops
        _same_with(pc, v, alt)
    _back_to_start(bp, ops, theta0)
    pc.refresh()
    assert pc.generation == 3 and id(pc._plan) == plan
    eager = pc.apply(v).clone()
    assert torch.equal(eager, first)
    _same_with(pc, v, alt)   # (puts the options back: the capture below is the default launches')
    out = torch.empty_like(v)
    g = pc.capture(v, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("inner", PAIRS, ids=["cheb-cheb", "mg2-mg1", "jacobi-cheb"])
@pytest.mark.parametrize("numerics", ["exact", "fast"])
@pytest.mark.parametrize("n", [16, 64])
def test_preconditioner_refresh_matches_fresh(n, numerics, inner):
    _refresh_walk(n, inner, numerics=numerics)


def test_preconditioner_refresh_csr_layout():
    _refresh_walk(16, PAIRS[1], layout="csr")


# n = 96: every fused launch of the apply is taken (csrc/: k_fsolve from n = 72, k_ftile 76, k_gtg_solve 78 for
# four sweeps, k_fpre / k_gal1 / k_gal1p 72, k_gtg_level0 78, the level-1 <PRO> ascents 80) -- the kernels that read the
# plan's by-value f_prm, the Chebyshev intervals and the multigrid levels a refresh rewrites
N_FUSED = 96
WALK_PAIRS = PAIRS + [("mg:1", "mg:1")]
WALK_IDS = ["cheb-cheb", "mg2-mg1", "jacobi-cheb", "mg1-mg1"]


def _per_sweep_opts(inner, numerics, n):
    """The launches the fused kernels replace, for _same_with."""
    if inner[0].startswith("mg"):
        if numerics == "fast":
            # below gal_fused_ok's n >= 72 the default level 1 is the stored Galerkin matrix, and the three matrix-free
            # launches of mg_galerkin_mf = 1 are another summation order of it (test_matrix_free_galerkin_level1)
            return dict(mg_fuse_l0=0, mg_galerkin_mf=1) if n >= 72 else dict(mg_fuse_l0=0)
        return dict(f_solve=0, f_tile=0, gtg_fused=0, mg_fuse_l0=0)   # (exact: k_gtg_level0 is the fused launch there)
    return dict(f_solve=0, f_tile=0, gtg_fused=0)


@pytest.mark.parametrize("inner", WALK_PAIRS, ids=WALK_IDS)
@pytest.mark.parametrize("numerics", ["exact", "fast"])
def test_preconditioner_refresh_matches_fresh_fused_sizes(numerics, inner):
    _refresh_walk(N_FUSED, inner, alt=_per_sweep_opts(inner, numerics, N_FUSED), numerics=numerics)


@pytest.mark.parametrize("inner", PAIRS[:2], ids=WALK_IDS[:2])
@pytest.mark.parametrize("numerics", ["exact", "fast"])
@pytest.mark.parametrize("n", [32, N_FUSED])
def test_refresh_follows_xi_eta_s_and_d_p(n, numerics, inner):
    """STEP_ALL: xi, eta_s and d_p change too (bp.xi, bp.eta_s, refill's d_p) -- the operators, the intervals and the
    apply are a freshly built preconditioner's, bit for bit, with the fused launches and with the per-sweep ones; and
    the way back to theta_0 restores the first apply."""
    bp, ops = _start(n)
    theta0 = [t.clone() for t in bp.theta_tables()]
    pc = _pc(ops, inner, numerics=numerics)
    v = torch.from_numpy(np.random.default_rng(n + 4).standard_normal(pc.shape[0])).cuda()
    first = pc.apply(v).clone()
    _step_to(bp, ops, STEP_ALL, n)
    pc.refresh()
    _, fops = _fresh(n, STEP_ALL)
    for name, M, ref in zip("AFDG", ops, fops):
        _same_values(M, ref, name)
    ref = _pc(fops, inner, numerics=numerics)
    _same_values(pc.GtG, ref.GtG, "Gt_G")
    _same_values(pc.GtFG, ref.GtFG, "Gt_F_G")
    assert (pc.inner_F.lmin, pc.inner_F.lmax, pc.inner_P.lmin, pc.inner_P.lmax) == \
        (ref.inner_F.lmin, ref.inner_F.lmax, ref.inner_P.lmin, ref.inner_P.lmax)
    got = pc.apply(v).clone()
    assert torch.equal(got, ref.apply(v))
    assert not torch.equal(got, first)
    alt = _per_sweep_opts(inner, numerics, n)
    _same_with(pc, v, alt)
    del ref, fops
    _back_to_start(bp, ops, theta0)
    pc.refresh()
    assert torch.equal(pc.apply(v), first)
    _same_with(pc, v, alt)


def test_explicit_chebyshev_bounds_stay_fixed():
    mp = _mp()
    n = 16
    bp, ops = _start(n)
    pc = mp.ApproxSchurPreconditioner(*ops[1:], inner_F=mp.InnerSolver("chebyshev", 4, lmin=0.1, lmax=2.5),
                                      inner_P=mp.InnerSolver("chebyshev", 4))
    _step_to(bp, ops, STEPS[2], n)
    pc.refresh()
    assert (pc.inner_F.lmin, pc.inner_F.lmax) == (0.1, 2.5)
    assert (pc._plan.inner_F.lmin, pc._plan.inner_F.lmax) == (0.1, 2.5)
    assert pc.inner_P.lmax == pc.GtG.gershgorin(pc.diag_P) == pc._plan.inner_P.lmax
    with pytest.raises(ValueError):
        pc.refresh(products="maybe")


# ------------------------------------------------------------------------------------------------ 5. in place
def _addresses(s, seen=None):
    """Every address a ctypes struct holds, through the structs it embeds or points to (an Mg's levels by count)."""
    from mp_block_preconditioners_amd import _lib
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, ctypes.Structure):
            out += _addresses(v)
        elif isinstance(v, ctypes.Array):
            out += [int(x or 0) for x in v]
        elif typ is ctypes.c_void_p:
            out.append(int(v or 0))
        elif isinstance(v, ctypes._Pointer):
            addr = ctypes.cast(v, ctypes.c_void_p).value or 0
            out.append(addr)
            if addr and typ._type_ is _lib.MgLevel:
                for l in range(s.nlevels):
                    out += _addresses(v[l])
            elif addr and issubclass(typ._type_, ctypes.Structure) and typ._type_ is not _lib.KernelOpts:
                out += _addresses(v.contents)
    return out


def test_refresh_is_in_place():
    n = 64
    bp, ops = _start(n)
    pc = _pc(ops, PAIRS[1], numerics="fast")
    v = torch.from_numpy(np.random.default_rng(0).standard_normal(pc.shape[0])).cuda()
    pc.apply(v)
    torch.cuda.synchronize()
    plan, before = id(pc._plan), _addresses(pc._plan)
    assert sum(1 for a in before if a) > 100      # both hierarchies' levels were walked
    base = torch.cuda.memory_allocated()
    for step in STEPS:
        _step_to(bp, ops, step, n)
        pc.refresh()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() <= base
        assert id(pc._plan) == plan
        assert _addresses(pc._plan) == before
    assert pc.generation == 3


# ------------------------------------------------------------------------------ 6. value-dependent decisions
def test_refresh_retakes_the_q13_sym_decision():
    mp = _mp()
    from mp_block_preconditioners_amd.csr import DeviceCSR
    n = 32
    _, ops = _start(n)
    F, D, G = ops[1:]
    GtG, Q = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)
    GtFG = DeviceCSR(Q.row_ptr, Q.col_idx, Q.val.clone(), Q.shape)      # the caller's own matrix (symmetric)
    kw = dict(inner_F=_inner("chebyshev:4"), inner_P=_inner("chebyshev:4"), numerics="fast",
              kernel_opts={"q13_sym": 1})
    pc = mp.ApproxSchurPreconditioner(F, D, G, GtG, GtFG, **kw)
    assert pc.kernel_opts.q13_sym == 1
    rng = np.random.default_rng(6)
    GtFG.val.mul_(torch.from_numpy(1.0 + 0.25 * rng.random(GtFG.nnz)).cuda())     # no longer symmetric
    pc.refresh(products="given")
    assert pc.kernel_opts.q13_sym == 0
    ref = mp.ApproxSchurPreconditioner(F, D, G, GtG, GtFG, **kw)
    assert ref.kernel_opts.q13_sym == 0
    v = torch.from_numpy(rng.standard_normal(pc.shape[0])).cuda()
    assert torch.equal(pc.apply(v), ref.apply(v))
    # symmetric again: the choice comes back
    GtFG.val.copy_(Q.val)
    pc.refresh(products="given")
    assert pc.kernel_opts.q13_sym == 1
    assert torch.equal(pc.apply(v), mp.ApproxSchurPreconditioner(F, D, G, GtG, GtFG, **kw).apply(v))


# --------------------------------------------------------------------------------------------------- 7. solve
def test_fgmres_history_after_refresh_matches_fresh():
    mp = _mp()
    n, step = 32, STEPS[2]
    _, fops = _fresh(n, step)
    xs = torch.from_numpy(np.random.default_rng(9).standard_normal(5 * n * n)).cuda()
    b = fops[0].matvec(xs)                                  # a consistent right-hand side (A is singular)
    bp, ops = _start(n)
    M = _pc(ops, PAIRS[1])
    h0 = []
    mp.fgmres(ops[0], b, M=M, tol=1e-8, maxiter=60, residuals=h0)   # (leaves a captured graph: refresh must drop it)
    _step_to(bp, ops, step, n)
    M.refresh()
    got, want = [], []
    x, info = mp.fgmres(ops[0], b, M=M, tol=1e-8, maxiter=60, residuals=got)
    xr, infor = mp.fgmres(fops[0], b, M=_pc(fops, PAIRS[1]), tol=1e-8, maxiter=60, residuals=want)
    print("fgmres after refresh: info", info, "fresh", infor, "iterations", len(got) - 1, "last", got[-1] / got[0])
    assert got == want and len(got) > 2 and got != h0
    assert info == infor
    assert torch.equal(x, xr)
