"""CPU checks of the any-size coarsening rule (mg.Multigrid(coarsen="any")) through its restatement
(tests/mg_any_restatement.py): the general 1D interpolation against oracle/mg_oracle.py's for even sizes, its structure
for odd ones, the Galerkin row widths the wide products must hold, and the cycle's contraction next to today's path."""
import numpy as np
import pytest
import scipy.sparse as sp

import mg_any_restatement as ra

ODD = [5, 7, 9, 11, 13, 23, 25, 47, 75, 125]


@pytest.fixture(scope="module")
def mo(oracle_built):
    from oracle import mg_oracle
    return mg_oracle


@pytest.mark.parametrize("nf", [6, 8, 16, 50, 94])
@pytest.mark.parametrize("kind", [ra.CELL, ra.NODE], ids=["cell", "node"])
def test_even_sizes_give_the_oracles_p1d(mo, nf, kind):
    got, ref = ra.p1d(nf, kind), mo.p1d(nf, kind)
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert np.array_equal(got.data.view(np.uint64), ref.data.view(np.uint64))


@pytest.mark.parametrize("nf", ODD)
@pytest.mark.parametrize("kind", [ra.CELL, ra.NODE], ids=["cell", "node"])
def test_odd_sizes_structure(nf, kind):
    P = ra.p1d(nf, kind)
    assert P.shape == (nf, nf // 2)
    plen = np.diff(P.indptr)
    assert plen.min() >= 1 and plen.max() <= 2
    for f in range(nf):   # the row sum in the stored order, exactly 1
        w = P.data[P.indptr[f]:P.indptr[f + 1]]
        assert (w[0] if len(w) == 1 else w[0] + w[1]) == 1.0, (f, w)
        assert np.all(w > 0.0)
        assert np.all(np.diff(P.indices[P.indptr[f]:P.indptr[f + 1]]) > 0)   # sorted, no duplicate (nc >= 2)
    R = sp.csr_matrix(P.T)
    rlen = np.diff(R.indptr)
    assert rlen.min() >= 3 and rlen.max() <= 5, rlen


def test_level_sizes_restated():
    assert ra.level_sizes(1000, 16) == [1000, 500, 250, 125, 62, 31, 15]
    assert ra.level_sizes(94, 16) == [94, 47, 23, 11]
    assert ra.level_sizes(23, 16) == [23, 11]
    assert ra.level_sizes(100, 8) == [100, 50, 25, 12, 6]
    assert ra.level_sizes(16, 16) == [16, 8]   # (at least one coarsening)


@pytest.mark.parametrize("n,widest", [(23, 75), (46, 86)])
def test_widest_galerkin_rows(mo, n, widest):
    """F's Galerkin rows below an odd level pass the 64-entry cap of the products (they must fit the wide forms' 128);
    the A P intermediates -- a triple refill's inner rows -- stay within 64."""
    from oracle.stokes_oracle import StokesSystem
    S = StokesSystem(n, 1.0, 100.0, 1.0)
    inner = []
    # (23, 11, 5): 75 at size 5; (46, 23, 11): 86 at size 11
    ops, _, _ = ra.hierarchy(S.F, n, mo.FIELDS_VELOCITY, coarsest=8 if n == 23 else 16, keep_inner=inner)
    got = max(int(np.diff(M.indptr).max()) for M, _ in ops[1:])
    assert got == widest
    assert got <= 128
    assert max(int(np.diff(M.indptr).max()) for M in inner) <= 64


def _eighth_ratio(ora, A, project_mean=False):
    return ra.contraction(ora, A, steps=8, seed=0, project_mean=project_mean)[-1]


def test_contraction_F_94_against_96(mo):
    """One V(2,2) cycle for F at eta_n = 100, coarsest 16: n = 94 (94, 47, 23, 11) against n = 96 under the unmodified
    oracle (96, 48, 24, 12).  A misplaced interpolation point, not roundoff, is what 1.25 x catches (measured 1.015 x)."""
    from oracle.stokes_oracle import StokesSystem
    S96 = StokesSystem(96, 1.0, 100.0, 1.0)
    r96 = _eighth_ratio(mo.MgOracle(S96.F, 96, mo.FIELDS_VELOCITY, coarsest=16), S96.F)
    S94 = StokesSystem(94, 1.0, 100.0, 1.0)
    ora = ra.MgAnyOracle(S94.F, 94, mo.FIELDS_VELOCITY, coarsest=16)
    assert [m for _, m in ora.ops] == [94, 47, 23, 11]
    r94 = _eighth_ratio(ora, S94.F)
    print(f"F contraction, 8th ratio: n=96 {r96:.4f}, n=94 {r94:.4f} ({r94 / r96:.3f} x)")
    assert r94 <= 1.25 * r96


def test_contraction_GtG_47_against_48(mo):
    """The same for Gt_G with its constant null space projected out: an odd level 0 costs a factor of about 1.9."""
    from oracle.stokes_oracle import StokesSystem
    S48 = StokesSystem(48, 1.0, 100.0, 1.0)
    r48 = _eighth_ratio(mo.MgOracle(S48.GtG, 48, mo.FIELDS_PRESSURE, coarsest=16), S48.GtG, project_mean=True)
    S47 = StokesSystem(47, 1.0, 100.0, 1.0)
    ora = ra.MgAnyOracle(S47.GtG, 47, mo.FIELDS_PRESSURE, coarsest=16)
    assert [m for _, m in ora.ops] == [47, 23, 11]
    r47 = _eighth_ratio(ora, S47.GtG, project_mean=True)
    print(f"Gt_G contraction, 8th ratio: n=48 {r48:.4f}, n=47 {r47:.4f} ({r47 / r48:.3f} x)")
    assert r47 <= 2.5 * r48


def test_python_level_sizes_and_argument_checks():
    """The package's own level_sizes under both rules (needs no GPU), and the keyword's validation."""
    from mp_block_preconditioners_amd import mg
    assert mg.level_sizes(1000, 16) == [1000, 500, 250, 125]
    assert mg.level_sizes(1000, 16, coarsen="even") == [1000, 500, 250, 125]
    assert mg.level_sizes(1000, 16, coarsen="any") == [1000, 500, 250, 125, 62, 31, 15]
    for n in (5, 23, 46, 47, 94, 100, 1002):
        for coarsest in (8, 16):
            assert mg.level_sizes(n, coarsest, coarsen="any") == ra.level_sizes(n, coarsest)
    with pytest.raises(ValueError, match="coarsen"):
        mg.level_sizes(64, 16, coarsen="odd")
    import mp_block_preconditioners_amd as mp
    assert mp.InnerSolver("mg", 1).coarsen == "even"
    assert mp.InnerSolver("mg", 1, coarsen="any").resolve(None, None).coarsen == "any"
