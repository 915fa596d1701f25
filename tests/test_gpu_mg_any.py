"""Multigrid on any grid size (mg.Multigrid(coarsen="any"), mpbp_mg_transfer_any_*, the wide products) against its CPU
restatement (tests/mg_any_restatement.py over oracle/mg_oracle.py and oracle/csr_oracle.c), bit for bit in exact
numerics: transfers, wide SpGEMM and refills, hierarchy, V-cycle under every kernel choice, the Schur apply, refresh;
fast numerics against the exact apply; FGMRES at n = 94 next to n = 96 under the default rule."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import mg_any_restatement as ra
from conftest import rel_inf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def _same_csr(dev, ref, what=""):
    got = dev.to_scipy()
    ref = sp.csr_matrix(ref)
    assert got.shape == ref.shape, what
    assert np.array_equal(got.indptr, ref.indptr), f"row_ptr differs {what}"
    assert np.array_equal(got.indices, ref.indices), f"col_idx differs {what}"
    assert np.array_equal(got.data.view(np.uint64), ref.data.view(np.uint64)), f"values differ {what}"


@functools.lru_cache(maxsize=None)
def _system(n, eta_n=100.0):
    """(preconditioner builder, (A, F, D, G), Gt_G on the device, the oracle's system) -- shared, never modified."""
    from oracle.stokes_oracle import StokesSystem, theta_tables
    mp = _mp()
    tables = theta_tables(n)
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
    bp.set_theta_tables(*tables)
    A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
    GtG, _ = mp.MultiphaseBlockPreconditioner.commutator_products(F, D, G)
    return bp, (A, F, D, G), GtG, StokesSystem(n, 1.0, eta_n, 1.0, tables=tables)


def _operators(n):
    mp = _mp()
    _, (A, F, D, G), GtG, S = _system(n)
    return ((F, S.F, mp.FIELDS_VELOCITY, "F"), (GtG, S.GtG, mp.FIELDS_PRESSURE, "Gt_G"))


@functools.lru_cache(maxsize=None)
def _restated_hierarchy(n, coarsest, name):
    _, _, _, S = _system(n)
    mp = _mp()
    M, fields = (S.F, mp.FIELDS_VELOCITY) if name == "F" else (S.GtG, mp.FIELDS_PRESSURE)
    inner = []
    ops, Ps, Rs = ra.hierarchy(M, n, fields, coarsest, keep_inner=inner)
    return ops, Ps, Rs, inner


# ------------------------------------------------------------------------------------------------ transfers
@pytest.mark.parametrize("n", [5, 7, 9, 11, 13, 23, 47, 94])
@pytest.mark.parametrize("which", ["P", "R"])
def test_transfer_any_bit_exact(n, which):
    """The smallest wraps (5, 7), both parities of nc, and an even n, where the rule is today's transfer."""
    mp = _mp()
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.mg import transfer
    w = _lib.MG_P if which == "P" else _lib.MG_R
    for fields in (mp.FIELDS_PRESSURE, mp.FIELDS_VELOCITY):
        got = transfer(n, fields, w, torch.device("cuda"), coarsen="any")
        _same_csr(got, ra.transfer(n, fields, which), f"n={n} {which}")
        if n % 2 == 0:
            today = transfer(n, fields, w, torch.device("cuda"))
            _same_csr(got, today.to_scipy(), "against the 2:1 transfer")


def test_transfer_any_argument_checks():
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.mg import transfer
    with pytest.raises(_lib.MpbpError, match="n >= 5"):
        transfer(4, ((0, 0),), _lib.MG_P, torch.device("cuda"), coarsen="any")
    with pytest.raises(ValueError, match="coarsen"):
        transfer(8, ((0, 0),), _lib.MG_P, torch.device("cuda"), coarsen="odd")
    with pytest.raises(_lib.MpbpError):   # the default rule still refuses an odd grid
        transfer(7, ((0, 0),), _lib.MG_P, torch.device("cuda"))


# ------------------------------------------------------------------------------------------------ wide products
def _dev(M):
    from mp_block_preconditioners_amd.csr import DeviceCSR
    M = sp.csr_matrix(M)
    M.sort_indices()
    return DeviceCSR.from_scipy(M)


def _blank(ref, fill=float("nan")):
    from mp_block_preconditioners_amd.csr import DeviceCSR
    return DeviceCSR(ref.row_ptr.clone(), ref.col_idx.clone(), torch.full_like(ref.val, fill), ref.shape)


def _refill_pair_wide(A, B, alpha, C):
    from mp_block_preconditioners_amd._lib import check, lib, stream_handle
    check(lib().mpbp_spgemm_refill_wide(ctypes.byref(A.cstruct()), ctypes.byref(B.cstruct()), alpha,
                                        ctypes.byref(C.cstruct()), stream_handle()))


def _refill_triple_wide(X, Y, Z, assoc, C):
    from mp_block_preconditioners_amd._lib import check, lib, stream_handle
    check(lib().mpbp_triple_refill_wide(ctypes.byref(X.cstruct()), ctypes.byref(Y.cstruct()), ctypes.byref(Z.cstruct()),
                                        assoc, 1.0, 1.0, ctypes.byref(C.cstruct()), stream_handle()))


def _check_products(X, Y, Z, expect_left_inner_ok):
    """Wide SpGEMM, pair refill and both triple associations of X Y Z (scipy CSR) against csr_oracle.spgemm."""
    from oracle import csr_oracle as co
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.csr import spgemm
    dX, dY, dZ = _dev(X), _dev(Y), _dev(Z)
    YZ = co.spgemm(Y, Z)
    right = co.spgemm(X, YZ)
    dYZ = spgemm(dY, dZ, wide=True)
    _same_csr(dYZ, YZ, "Y Z")
    got = spgemm(dX, dYZ, wide=True)
    _same_csr(got, right, "X (Y Z)")
    C = _blank(got)
    _refill_pair_wide(dX, dYZ, 1.0, C)
    assert np.array_equal(_bits(C.val), right.data.view(np.uint64)), "pair refill"
    C = _blank(got)
    _refill_triple_wide(dX, dY, dZ, _lib.ASSOC_RIGHT, C)
    assert np.array_equal(_bits(C.val), right.data.view(np.uint64)), "triple refill, right"
    XY = co.spgemm(X, Y)
    C = _blank(got)
    if expect_left_inner_ok:
        assert int(np.diff(XY.indptr).max()) <= 64
        left = co.spgemm(XY, Z)
        assert np.array_equal(left.indices, right.indices)
        _refill_triple_wide(dX, dY, dZ, _lib.ASSOC_LEFT, C)
        assert np.array_equal(_bits(C.val), left.data.view(np.uint64)), "triple refill, left"
    else:   # (X Y)'s rows pass the inner cap: refused by name
        assert int(np.diff(XY.indptr).max()) > 64
        with pytest.raises(_lib.MpbpError, match="inner row wider than 64"):
            _refill_triple_wide(dX, dY, dZ, _lib.ASSOC_LEFT, C)
    return int(np.diff(right.indptr).max())


@pytest.mark.parametrize("n,coarsest,widest", [(23, 8, 75), (46, 16, 86)])
def test_wide_products_on_the_F_hierarchies(n, coarsest, widest):
    """R (A P) of every level of the two smallest hierarchies with an F row over 64 entries.  The left association's
    inner rows (R A) stay within 64 on level 0 of n = 46 only (58); elsewhere they reach 106-190 and are refused."""
    ops, Ps, Rs, _ = _restated_hierarchy(n, coarsest, "F")
    seen = 0
    for l in range(len(Ps)):
        seen = max(seen, _check_products(Rs[l], ops[l][0], Ps[l], expect_left_inner_ok=(n == 46 and l == 0)))
    assert seen == widest


def _exact_width_case():
    """X (5 x 18), Y (18 x 18), Z (18 x 300): the rows of X Y Z hold exactly 65, 127, 128 and 128 entries and row 4
    none.  Block r of Z's rows covers its W columns (a seeded permutation) in slices of 30 stepping 25, so columns
    are hit by several products; Y couples neighbouring rows of a block, so the inner rows (Y Z: <= 55, X Y: <= 6)
    stay within 64."""
    rng = np.random.default_rng(128)
    widths = [65, 127, 128, 128]
    nz = sum(-(-w // 25) for w in widths)
    X, Y, Z = sp.lil_matrix((5, nz)), sp.lil_matrix((nz, nz)), sp.lil_matrix((nz, 300))
    row = 0
    for r, W in enumerate(widths):
        cols = rng.permutation(300)[:W]
        k = -(-W // 25)
        for j in range(k):
            sl = cols[25 * j:min(25 * j + 30, W)]
            Z[row + j, sl] = rng.standard_normal(len(sl))
            Y[row + j, row + j] = rng.standard_normal()
            Y[row + j, row + (j + 1) % k] = rng.standard_normal()
            X[r, row + j] = rng.standard_normal()
        row += k
    return sp.csr_matrix(X), sp.csr_matrix(Y), sp.csr_matrix(Z), widths


def test_wide_products_exact_widths():
    from oracle import csr_oracle as co
    X, Y, Z, widths = _exact_width_case()
    assert list(np.diff(co.spgemm(X, co.spgemm(Y, Z)).indptr)) == widths + [0]
    assert _check_products(X, Y, Z, expect_left_inner_ok=True) == 128


def test_wide_products_refusals():
    """A 129-entry output row and a 65-entry inner row name their cap, and the refused row is not written."""
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd.csr import spgemm
    one = _dev(np.ones((1, 1)))
    row129, row65, col65, eye65 = _dev(np.ones((1, 129))), _dev(np.ones((1, 65))), _dev(np.ones((65, 1))), _dev(sp.identity(65))
    with pytest.raises(_lib.MpbpError, match="wider than 128"):
        spgemm(one, row129, wide=True)
    C = _blank(row129, 7.0)
    with pytest.raises(_lib.MpbpError, match="wider than 128"):
        _refill_pair_wide(one, row129, 1.0, C)
    assert bool(torch.all(C.val == 7.0))
    C = _blank(row129, 7.0)
    with pytest.raises(_lib.MpbpError, match="wider than 128"):
        _refill_triple_wide(one, one, row129, _lib.ASSOC_RIGHT, C)
    assert bool(torch.all(C.val == 7.0))
    # inner rows: (X Y) of 65 entries under a one-entry output row; (Y Z) of 65 entries under a 65-entry output row
    C = _blank(one, 7.0)
    with pytest.raises(_lib.MpbpError, match="inner row wider than 64"):
        _refill_triple_wide(one, row65, col65, _lib.ASSOC_LEFT, C)
    assert bool(torch.all(C.val == 7.0))
    C = _blank(row65, 7.0)
    with pytest.raises(_lib.MpbpError, match="inner row wider than 64"):
        _refill_triple_wide(one, row65, eye65, _lib.ASSOC_RIGHT, C)
    assert bool(torch.all(C.val == 7.0))
    # the 64-wide entry points keep their cap and their words
    with pytest.raises(_lib.MpbpError, match="wider than 64"):
        spgemm(one, row65)
    _same_csr(spgemm(one, row65, wide=True), np.ones((1, 65)))


# ------------------------------------------------------------------------------------------ hierarchy and cycle
@functools.lru_cache(maxsize=None)
def _multigrid(n, coarsest, name):
    mp = _mp()
    M, _, fields, _ = [o for o in _operators(n) if o[3] == name][0]
    return mp.Multigrid(M, n, fields, coarsest=coarsest, coarsen="any")


@pytest.mark.parametrize("coarsest", [8, 16])
@pytest.mark.parametrize("n", [23, 46, 47, 94])
def test_hierarchy_any_bit_exact(n, coarsest):
    from oracle.schur_oracle import gershgorin
    from oracle import mg_oracle as mo
    for _, _, _, name in _operators(n):
        mg = _multigrid(n, coarsest, name)
        ops, Ps, Rs, _ = _restated_hierarchy(n, coarsest, name)
        assert mg.sizes == [m for _, m in ops] == ra.level_sizes(n, coarsest)
        for l, (Ml, _) in enumerate(ops):
            _same_csr(mg.ops[l], Ml, f"{name} level {l}")
            assert np.array_equal(_bits(mg.diags[l]), np.asarray(Ml.diagonal(), dtype=np.float64).view(np.uint64))
            ref = gershgorin(Ml, np.asarray(Ml.diagonal()))
            assert abs(mg.bounds[l][1] - ref) <= 1e-12 * ref
        for l in range(len(Ps)):
            _same_csr(mg.P[l], Ps[l], f"{name} P {l}")
            _same_csr(mg.R[l], Rs[l], f"{name} R {l}")
        # the coarse inverse: the same LAPACK pseudo-inverse of the same bits (identical up to the library's threading)
        pinv = np.linalg.pinv(ops[-1][0].toarray(), rcond=mo.COARSE_RCOND)
        assert np.max(np.abs(mg.coarse_inv_host - pinv)) <= 1e-12 * np.max(np.abs(pinv))
        assert all(V is None for V in mg.svls)   # no stencil-values layout on these levels


@pytest.mark.parametrize("n", [23, 46, 47, 94])
def test_solve_any_bit_exact_under_every_kernel_choice(n):
    """Two V(2,2) cycles (the second from a nonzero iterate) against the restated cycle: transfers matrix-free or
    stored, small levels on the grouped kernel or the row kernels, the fused residual + restriction on or off."""
    for M, Mh, fields, name in _operators(n):
        mg = _multigrid(n, 8, name)
        ora = ra.MgAnyOracle(Mh, n, fields, cycles=2, coarsest=8, bounds=mg.bounds, coarse_inv=mg.coarse_inv_host)
        rng = np.random.default_rng(n)
        b, sub = rng.standard_normal(M.shape[0]), rng.standard_normal(M.shape[0])
        ref, ref_sub = ora.solve(b), ora.solve(b, sub=sub)
        saved = (mg._mg.cycles, mg.kernel_opts.mg_mf_transfer, mg.kernel_opts.mg_group_rows, mg.kernel_opts.mg_fuse_small)
        mg._mg.cycles = 2
        try:
            for mf in (1, 0):
                for grp in (65536, 0):
                    for fuse in (1, 0):
                        mg.kernel_opts.mg_mf_transfer, mg.kernel_opts.mg_group_rows = mf, grp
                        mg.kernel_opts.mg_fuse_small = fuse
                        what = f"{name} n={n} mf={mf} grp={grp} fuse={fuse}"
                        assert np.array_equal(_bits(mg.solve(_cuda(b))), _bits(ref)), what
                        assert np.array_equal(_bits(mg.solve(_cuda(b), sub=_cuda(sub))), _bits(ref_sub)), what
        finally:
            (mg._mg.cycles, mg.kernel_opts.mg_mf_transfer, mg.kernel_opts.mg_group_rows,
             mg.kernel_opts.mg_fuse_small) = saved


# ------------------------------------------------------------------------------------------------ Schur apply
def _inner(coarsest):
    return _mp().InnerSolver("mg", 1, coarsen="any", coarsest=coarsest)


def _oracle_apply(S, pc, v):
    """approx_schur_op (solve.py:257-277) with the restated cycles as both inner inverses (schur_oracle's order)."""
    from oracle import csr_oracle as co
    mF, mP = pc.mg_F, pc.mg_P
    oF = ra.MgAnyOracle(S.F, mF.n, mF.fields, mF.pre, mF.post, mF.cycles, bounds=mF.bounds,
                        coarse_inv=mF.coarse_inv_host, coarsest=mF.coarsest)
    oP = ra.MgAnyOracle(S.GtG, mP.n, mP.fields, mP.pre, mP.post, mP.cycles, bounds=mP.bounds,
                        coarse_inv=mP.coarse_inv_host, coarsest=mP.coarsest)
    nu = S.F.shape[0]
    Finv_v = oF.solve(v[:nu])
    x_a = oP.solve(co.spmv(S.D, Finv_v, v[nu:], mode=1))
    x_p = oP.solve(co.spmv(S.GtFG, x_a))
    return np.concatenate([oF.solve(co.spmv(S.G, x_p), sub=Finv_v), x_p])


@functools.lru_cache(maxsize=None)
def _exact_pc(n, coarsest):
    mp = _mp()
    _, (A, F, D, G), _, _ = _system(n)
    return mp.ApproxSchurPreconditioner(F, D, G, inner_F=_inner(coarsest), inner_P=_inner(coarsest))


# (n, coarsest): odd level 0; even n with an odd level 1; (100, 50, 25, 12, 6) with the odd level below level 1
@pytest.mark.parametrize("n,coarsest", [(47, 16), (94, 16), (100, 8)])
def test_schur_apply_any_exact_bit_exact(n, coarsest):
    _, _, _, S = _system(n)
    pc = _exact_pc(n, coarsest)
    assert pc.mg_F.sizes == pc.mg_P.sizes == ra.level_sizes(n, coarsest) and pc.mg_F.coarsen == "any"
    v = np.random.default_rng(n).standard_normal(pc.shape[0])
    ref = _oracle_apply(S, pc, v)
    assert np.array_equal(_bits(pc.apply(_cuda(v))), _bits(ref))
    vd, out = _cuda(v), torch.empty(pc.shape[0], dtype=torch.float64, device="cuda")
    g = pc.capture(vd, out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(ref))


# n = 81: odd and above every fused level-0 / level-1 kernel's minimum (72-82), so each of their gates must fall back
@pytest.mark.parametrize("n,coarsest", [(94, 16), (100, 8), (81, 16)])
def test_schur_apply_any_fast(n, coarsest):
    """Fast numerics against the exact apply under tests/test_gpu_mg_1024.py's rule: max(1e-12, 4 x floor), the floor
    being the exact apply's own response to a one-ulp relative perturbation of its input; and bit-equal to the same
    apply with the fused level-0 and level-1 kernels switched off."""
    mp = _mp()
    _, (A, F, D, G), _, _ = _system(n)
    exact = _exact_pc(n, coarsest)
    fast = mp.ApproxSchurPreconditioner(F, D, G, exact.GtG, exact.GtFG, inner_F=_inner(coarsest),
                                        inner_P=_inner(coarsest), numerics="fast")
    v = np.random.default_rng(n + 1).standard_normal(exact.shape[0])
    ref = exact.apply(_cuda(v)).cpu().numpy()
    sign = np.where(np.random.default_rng(3).random(v.size) < 0.5, -1.0, 1.0)
    floor = rel_inf(exact.apply(_cuda(v * (1.0 + sign * 2.0 ** -52))).cpu().numpy(), ref)
    got = fast.apply(_cuda(v)).cpu().numpy()
    err = rel_inf(got, ref)
    print(f"n={n}: fast vs exact {err:.3e}, one-ulp floor {floor:.3e}")
    assert floor > 0.0
    assert err <= max(1e-12, 4.0 * floor), (err, floor)
    # the fused launches switched back to the launches they replace (tests/test_gpu_fused_params.py's toggles): level
    # 0's k_fpre / k_gtg_level0 / tile-pair ascent off, level 1 as three launches instead of k_gal1 / k_gal1p.  (The
    # stored level 1, mg_galerkin_mf = 0, is another summation order of the same operator -- not these bits.)
    fast.set_kernel_opts(mg_fuse_l0=0, mg_galerkin_mf=1)
    plain = fast.apply(_cuda(v)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(plain)), rel_inf(got, plain)
    fast.set_kernel_opts(mg_galerkin_mf=0)
    stored = fast.apply(_cuda(v)).cpu().numpy()
    assert rel_inf(stored, ref) <= max(1e-12, 4.0 * floor), (rel_inf(stored, ref), floor)


# ---------------------------------------------------------------------------------------------------- refresh
def _smooth_tables(n):
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * x) * np.sin(4 * np.pi * y)
    return f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx)


@pytest.mark.parametrize("n", [46, 94])
def test_refresh_any_matches_fresh_build(n):
    """update_theta_tables + refill, then Multigrid.refresh (the wide triple refill): every level, diagonal, bound and
    the coarse inverse equal a fresh build's bit for bit, at the addresses the hierarchy held before."""
    mp = _mp()

    def build(tables, eta_n, c, d_u):
        bp = mp.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
        if tables is not None:
            bp.set_theta_tables(*tables)
        return bp, bp.get_big_A_matrix(c=c, d_u=d_u)
    bp, (A, _, F, D, G) = build(None, 100.0, 1.0, -1.0)
    mg = mp.Multigrid(F, n, mp.FIELDS_VELOCITY, coarsest=8, coarsen="any")
    assert max(int(np.diff(M.row_ptr_host).max()) for M in mg.ops) > 64   # the wide refill is needed
    ptrs = [M.val.data_ptr() for M in mg.ops] + [d.data_ptr() for d in mg.diags] + [mg.coarse_inv.val.data_ptr()]
    tabs = _smooth_tables(n)
    bp.update_theta_tables(*tabs)
    bp.eta_n = 1.0e4
    bp.refill(A, F, D, G, c=4.0, d_u=-0.5)
    mg.refresh()
    _, (_, _, F2, _, _) = build(tabs, 1.0e4, 4.0, -0.5)
    ref = mp.Multigrid(F2, n, mp.FIELDS_VELOCITY, coarsest=8, coarsen="any")
    assert mg.sizes == ref.sizes and mg.bounds == ref.bounds
    for l in range(mg.nlevels):
        assert torch.equal(mg.ops[l].col_idx, ref.ops[l].col_idx) and torch.equal(mg.ops[l].val, ref.ops[l].val), l
        assert torch.equal(mg.diags[l], ref.diags[l]), l
    assert np.array_equal(mg.coarse_inv_host, ref.coarse_inv_host)
    assert ptrs == [M.val.data_ptr() for M in mg.ops] + [d.data_ptr() for d in mg.diags] + [mg.coarse_inv.val.data_ptr()]
    b = _cuda(np.random.default_rng(3).standard_normal(F.shape[0]))
    assert torch.equal(mg.solve(b), ref.solve(b))


# ----------------------------------------------------------------------------------------------------- FGMRES
def test_fgmres_converges_at_94_like_96():
    """eta_n = 100, tol 1e-8, mg:1 / mg:1, fast numerics: n = 94 (94, 47, 23, 11; coarsen="any") against n = 96 under
    the default rule (96, 48, 24, 12).  The margin: FGMRES's count follows the inner solves' contraction like
    1 / log(1 / rho); the restated cycle's rho for F is 0.0898 at 94 against 0.0885 at 96 (1.015 x, asserted within
    1.25 x in tests/test_mg_any_restatement.py), Gt_G's is the same (0.0463), and ln 0.0885 / ln (1.25 * 0.0885) = 1.10.
    So at most 10 % more iterations, plus 2 for the count's granularity and the 2 % finer grid at 96."""
    mp = _mp()
    its = {}
    for n, coarsen in ((96, "even"), (94, "any")):
        _, (A, F, D, G), _, _ = _system(n)
        _, b = mp.manufactured_problem(n, etan=100.0, etas=1.0)
        inner = mp.InnerSolver("mg", 1, coarsen=coarsen)
        pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=inner, inner_P=inner, numerics="fast")
        hist = []
        _, info = mp.fgmres(A, _cuda(b), M=pc, tol=1e-8, maxiter=150, residuals=hist)
        its[n] = len(hist) - 1
        assert info == 0, (n, its)
    print(f"FGMRES iterations: n=96 {its[96]}, n=94 {its[94]}")
    assert its[94] <= 1.10 * its[96] + 2, its


# --------------------------------------------------------------------------------------------------- defaults
def test_defaults_unchanged():
    mp = _mp()
    from mp_block_preconditioners_amd import mg
    assert mg.level_sizes(1000, 16) == [1000, 500, 250, 125]
    assert mg.level_sizes(1000, 16, coarsen="any") == [1000, 500, 250, 125, 62, 31, 15]
    F = _operators(94)[0][0]
    with pytest.raises(ValueError, match="exceed the dense inverse's 8192"):
        mp.Multigrid(F, 94, mp.FIELDS_VELOCITY)
    with pytest.raises(ValueError, match='coarsen="any"'):   # the hint
        mp.Multigrid(F, 94, mp.FIELDS_VELOCITY)
    with pytest.raises(ValueError, match="even grid"):
        mp.Multigrid(_operators(47)[0][0], 47, mp.FIELDS_VELOCITY)
    from mp_block_preconditioners_amd.distributed import DistributedSchurPreconditioner, PartitionedMultigrid
    with pytest.raises(ValueError, match="row partition"):
        DistributedSchurPreconditioner(32, 1.0, 100.0, 1.0, inner_F=mp.InnerSolver("mg", 1, coarsen="any"))
    with pytest.raises(ValueError, match="row partition"):
        PartitionedMultigrid(_multigrid(46, 16, "Gt_G"), None, 1)
