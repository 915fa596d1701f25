"""The CPU restatement of the block forms (tests/block_forms_restatement.py) against dense linear algebra: the signs of
each composition, the block matrix each form inverts, and the relations between the forms."""
import functools

import numpy as np
import pytest

import block_forms_restatement as bf
from conftest import rel_inf

TOL_EXACT = 1e-8   # the project's bar for exact inner solves (tests/test_oracle_golden.py)
PRMS = {"unit": (1.0, 1.0, 1.0, 1.0, -1.0), "eta100": (1.0, 100.0, 1.0, 1.0, -1.0)}   # xi, eta_n, eta_s, c, d_u
SIZES = [4, 5, 8]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _dense(n, prm):
    """The oracle's system with dense F^-1, pinv(Gt_G) and S~^-1 = pinv(Gt_G) Gt_F_G pinv(Gt_G)."""
    from oracle.stokes_oracle import StokesSystem
    S = StokesSystem(n, *PRMS[prm])
    Fd, Dd, Gd = S.F.toarray(), S.D.toarray(), S.G.toarray()
    Finv = np.linalg.inv(Fd)
    Pinv = np.linalg.pinv(S.GtG.toarray(), rcond=1e-11)
    Sinv = Pinv @ S.GtFG.toarray() @ Pinv
    return S, Fd, Dd, Gd, Finv, Pinv, Sinv


def _vector(n, S, zero_mean=False):
    v = np.random.default_rng(17 * n).standard_normal(S.A.shape[0])
    if zero_mean:
        nu = S.F.shape[0]
        v[nu:] -= v[nu:].mean()
    return v


def _exact(form, n, prm, v):
    from oracle.schur_oracle import Inner
    S, _, _, _, Finv, Pinv, _ = _dense(n, prm)
    return bf.apply(form, S.F, S.D, S.G, S.GtG, S.GtFG, v, Inner("exact"), Inner("exact"),
                    F_inv=lambda r: Finv @ r, GtG_inv=lambda r: Pinv @ r)


@pytest.mark.parametrize("prm", list(PRMS))
@pytest.mark.parametrize("n", SIZES)
def test_exact_inner_solves_equal_the_dense_formulas(n, prm, oracle_built):
    S, Fd, Dd, Gd, Finv, Pinv, Sinv = _dense(n, prm)
    nu = Fd.shape[0]
    v = _vector(n, S)
    v_u, v_p = v[:nu], v[nu:]
    y = Finv @ v_u
    dense = {}
    x_p = Sinv @ (Dd @ y + v_p)
    dense["full"] = np.concatenate([y - Finv @ (Gd @ x_p), x_p])
    dense["lower"] = np.concatenate([y, x_p])
    x_p = Sinv @ v_p
    dense["upper"] = np.concatenate([Finv @ (v_u - Gd @ x_p), x_p])
    dense["diagonal"] = np.concatenate([y, x_p])
    for form in bf.FORMS:
        assert rel_inf(_exact(form, n, prm, v), dense[form]) <= TOL_EXACT, form
    # the signs matter: the forms differ from one another by far more than the bar
    assert rel_inf(dense["upper"], dense["diagonal"]) > 1e-3 and rel_inf(dense["lower"], dense["diagonal"]) > 1e-3
    assert rel_inf(dense["full"], dense["upper"]) > 1e-3


@pytest.mark.parametrize("prm", list(PRMS))
@pytest.mark.parametrize("n", SIZES)
def test_each_form_inverts_its_block_matrix(n, prm, oracle_built):
    """[[F, G], [0, S]] upper(v) = v and [[F, 0], [-D, S]] lower(v) = v for zero-mean v_p (the range of the singular S),
    with S = pinv(S~^-1); the diagonal form likewise with both off-diagonal blocks zero."""
    S, Fd, Dd, Gd, _, _, Sinv = _dense(n, prm)
    nu, npr = Fd.shape[0], Sinv.shape[0]
    Sd = np.linalg.pinv(Sinv, rcond=1e-11)
    assert np.linalg.matrix_rank(Sinv, tol=1e-11 * np.linalg.norm(Sinv, 2)) == npr - 1
    v = _vector(n, S, zero_mean=True)
    Z = np.zeros((nu, npr))
    blocks = {"upper": np.block([[Fd, Gd], [Z.T, Sd]]), "lower": np.block([[Fd, Z], [-Dd, Sd]]),
              "diagonal": np.block([[Fd, Z], [Z.T, Sd]])}
    for form, M in blocks.items():
        assert rel_inf(M @ _exact(form, n, prm, v), v) <= TOL_EXACT, form


@pytest.mark.parametrize("n", [5, 8])
def test_full_is_the_oracle_apply_and_the_forms_share_their_parts(n, oracle_built):
    """Sweeping inner solves: form="full" is oracle.schur_oracle.approx_schur_apply bit for bit; lower's pressure part is
    full's; lower's and diagonal's velocity parts are inner_solve(F, v_u); diagonal's pressure part is upper's."""
    from oracle.schur_oracle import Inner, approx_schur_apply, diagonal, gershgorin, inner_solve
    S = _dense(n, "eta100")[0]
    nu = S.F.shape[0]
    dF, dP = diagonal(S.F), diagonal(S.GtG)
    lF, lP = gershgorin(S.F, dF), gershgorin(S.GtG, dP)
    v = _vector(n, S)
    for iF, iP in ((Inner("chebyshev", 4, lF / 30, lF), Inner("chebyshev", 3, lP / 30, lP)),
                   (Inner("jacobi", 3), Inner("jacobi", 2))):
        out = {form: bf.apply(form, S.F, S.D, S.G, S.GtG, S.GtFG, v, iF, iP) for form in bf.FORMS}
        ref = approx_schur_apply(S.F, S.D, S.G, S.GtG, S.GtFG, v, iF, iP)
        assert np.array_equal(_bits(out["full"]), _bits(ref))
        assert np.array_equal(_bits(out["lower"][nu:]), _bits(out["full"][nu:]))
        assert np.array_equal(_bits(out["diagonal"][nu:]), _bits(out["upper"][nu:]))
        y = inner_solve(S.F, dF, iF, np.ascontiguousarray(v[:nu]))
        assert np.array_equal(_bits(out["lower"][:nu]), _bits(y))
        assert np.array_equal(_bits(out["diagonal"][:nu]), _bits(y))
        assert not np.array_equal(_bits(out["upper"][:nu]), _bits(y))


def test_check_form_refuses_unknown_names():
    from mp_block_preconditioners_amd import solve
    assert solve.FORMS == ("full", "upper", "lower", "diagonal") == bf.FORMS
    for form in solve.FORMS:
        assert solve._check_form(form) == form
    for bad in ("bogus", "Upper", "", None, 1):
        with pytest.raises(ValueError, match="full.*upper.*lower.*diagonal"):
            solve._check_form(bad)
    with pytest.raises(ValueError):
        bf.apply("bogus", *([None] * 8))


def test_plan_mirror_carries_the_form():
    from mp_block_preconditioners_amd import _lib
    assert (_lib.FORM_FULL, _lib.FORM_UPPER, _lib.FORM_LOWER, _lib.FORM_DIAGONAL) == (0, 1, 2, 3)
    assert _lib.SchurPlan._fields_[-1][0] == "form" and _lib.SchurPlan().form == _lib.FORM_FULL
