"""CPU checks of the refresh path's host logic: the slot permutation StencilValues keeps for its refill (mg.py), and
the two values-only product entry points' declarations."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")


def _periodic_operator(m, nf, rng):
    """nf stacked m x m periodic fields, every row the same 5-point offsets within its field plus one coupling to the
    next field, random values."""
    N = m * m
    rows, cols = [], []
    for f in range(nf):
        for r in range(m):
            for c in range(m):
                i = f * N + r * m + c
                for dr, dc in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
                    rows.append(i)
                    cols.append(f * N + ((r + dr) % m) * m + (c + dc) % m)
                rows.append(i)
                cols.append(((f + 1) % nf) * N + r * m + c)
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(nf * N, nf * N))
    A.sort_indices()
    return A


@pytest.mark.parametrize("nf", [1, 2])
def test_stencil_values_gather_is_the_build_permutation(nf):
    from mp_block_preconditioners_amd.mg import _stencil_values_arrays, stencil_values_arrays
    rng = np.random.default_rng(nf)
    m = 8
    A = _periodic_operator(m, nf, rng)
    args = (torch.from_numpy(A.indptr.astype(np.int32)), torch.from_numpy(A.indices.astype(np.int32)))
    val = torch.from_numpy(A.data.copy())
    full = _stencil_values_arrays(*args, val, nf, m)
    assert full is not None and len(stencil_values_arrays(*args, val, nf, m)) == 5
    vals, gather = full[3], full[5]
    assert gather.dtype == torch.int32 and gather.numel() == val.numel()
    assert np.array_equal(np.sort(gather.numpy()), np.arange(val.numel()))
    assert torch.equal(vals, val[gather.long()])
    # new values through the kept permutation == a fresh build's slot-major array (what StencilValues.refill does)
    new = torch.from_numpy(rng.standard_normal(val.numel()))
    out = torch.empty_like(vals)
    torch.index_select(new, 0, gather, out=out)
    assert torch.equal(out, _stencil_values_arrays(*args, new, nf, m)[3])


def test_refill_entry_points_are_declared():
    from mp_block_preconditioners_amd import _lib
    L = _lib.lib()
    for name in ("mpbp_spgemm_refill", "mpbp_triple_refill"):
        assert name in _lib.exported_symbols() and hasattr(L, name)
    assert (_lib.ASSOC_LEFT, _lib.ASSOC_RIGHT) == (0, 1)
    # host-side argument checks run before anything is launched
    one = _lib.Csr(1, 1, 0, None, None, None)
    import ctypes
    assert L.mpbp_spgemm_refill(ctypes.byref(one), ctypes.byref(one), 1.0, ctypes.byref(one), None) < 0
    assert b"invalid csr" in L.mpbp_last_error()
