"""mpbp_stokes_apply_part: the header declares it, the library exports it, every refusal comes back as its error code
with a message in mpbp_last_error() before any HIP call (host arrays stand in for the vectors: they are never
dereferenced, and y keeps its sentinel), and without a partition (part = NULL, halo = 0) it is mpbp_stokes_apply."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG, ERR_OVERFLOW = -1, -3
STORE, ADD, RESID, FAST = 0, 1, 2, 0x100
SENTINEL = -7.25


@pytest.fixture(scope="module")
def L():
    from mp_block_preconditioners_amd import _lib
    return _lib.lib()


def test_declared_and_exported(L):
    from mp_block_preconditioners_amd import _lib
    with open(os.path.join(ROOT, "include", "mpbp.h")) as f:
        src = f.read()
    assert re.search(r"\bint\s+mpbp_stokes_apply_part\s*\(\s*const\s+mpbp_stokes_params\s*\*", src)
    assert "mpbp_stokes_apply_part" in _lib.exported_symbols()
    fn = getattr(L, "mpbp_stokes_apply_part")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10


def _call(L, n=8, mode=STORE, part=(2, 4, 1, 0, 0, 0), prm=True, cell=True, uface=True, vface=True, x=True, z=None,
          y=True, alias=False):
    """part: (r0, rows, halo, which, ext, oh) or None.  Returns (rc, y unchanged)."""
    from mp_block_preconditioners_amd import _lib
    p = _lib.StokesParams(n, 1.0, 100.0, 1.0, 1.0, -1.0, 1.0, -1.0)
    buf = [np.full(8, SENTINEL) for _ in range(6)]
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) for b in buf]
    pick = lambda on, q: q if on else None
    rp = _lib.RowPart(*part) if part is not None else None
    rc = L.mpbp_stokes_apply_part(ctypes.byref(p) if prm else None, pick(cell, ptrs[0]), pick(uface, ptrs[1]),
                                  pick(vface, ptrs[2]), ctypes.byref(rp) if rp is not None else None, mode,
                                  pick(x, ptrs[3]), pick(z, ptrs[4]), ptrs[3] if alias else pick(y, ptrs[5]), None)
    return rc, all(np.all(b == SENTINEL) for b in buf)


# what mpbp_stokes_apply refuses, with a valid partition, with halo = 0 and with no partition
COMMON = [
    (dict(prm=False), "parameters"), (dict(cell=False), "tables"), (dict(uface=False), "tables"),
    (dict(vface=False), "tables"), (dict(x=False), "vectors"), (dict(y=False), "vectors"),
    (dict(alias=True), "vectors"), (dict(alias=True, mode=FAST), "vectors"),
    (dict(mode=ADD), "vectors"), (dict(mode=RESID), "vectors"), (dict(mode=ADD | FAST), "vectors"),
    (dict(n=2, part=(0, 2, 1, 0, 0, 0)), "n >= 3"), (dict(n=0), "n >= 3"), (dict(n=-4), "n >= 3"),
    (dict(mode=3), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(mode=FAST | 7), "unknown mode"),
    (dict(mode=0x200), "unknown mode"),
]


@pytest.mark.parametrize("how", ["part", "halo0", "null"])
@pytest.mark.parametrize("kw,word", COMMON,
                         ids=lambda v: "-".join(f"{k}{w}" for k, w in v.items()) if isinstance(v, dict) else None)
def test_common_refusals(L, kw, word, how):
    kw = dict(kw)
    if how == "halo0":
        kw["part"] = (0, 8, 0, 0, 0, 0)
    elif how == "null":
        kw["part"] = None
    rc, untouched = _call(L, **kw)
    assert rc == ERR_ARG and untouched
    msg = L.mpbp_last_error().decode()
    assert msg.startswith("stokes_apply") and word in msg, msg


# (r0, rows, halo, which, ext, oh) on an n = 8 grid
BAD_PARTS = [
    ((2, 4, 1, 3, 0, 0), "which"), ((2, 4, 1, 3, 1, 0), "which"),       # which = 3: no ghost output
    ((2, 4, 1, 0, 1, 0), "ext"), ((2, 4, 2, 1, 1, 0), "ext"), ((2, 4, 1, 2, -1, 0), "ext"),   # a non-zero ext
    ((2, 4, 1, 4, 0, 0), "which"), ((2, 4, 1, -1, 0, 0), "which"), ((2, 4, 1, 99, 0, 0), "which"),
    ((2, 0, 1, 0, 0, 0), "rows"), ((2, -3, 1, 0, 0, 0), "rows"),        # rows < 1
    ((-1, 4, 1, 0, 0, 0), "r0"),                                        # r0 < 0
    ((5, 4, 1, 0, 0, 0), "partition"), ((0, 9, 1, 0, 0, 0), "partition"), ((8, 1, 1, 0, 0, 0), "partition"),   # past n
    ((2, 1, 2, 0, 0, 0), "halo"), ((0, 4, 5, 0, 0, 0), "halo"),         # halo > rows
    ((2, 4, 1, 0, 0, 2), "oh"), ((2, 4, 2, 0, 0, 1), "oh"), ((2, 4, 1, 0, 0, -1), "oh"),   # oh other than 0 or halo
]


@pytest.mark.parametrize("mode", [STORE, ADD, RESID | FAST])
@pytest.mark.parametrize("part,word", BAD_PARTS, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else v)
def test_partition_refusals(L, part, word, mode):
    rc, untouched = _call(L, part=part, mode=mode, z=True)
    assert rc == ERR_ARG and untouched
    msg = L.mpbp_last_error().decode()
    assert msg.startswith("stokes_apply_part") and word in msg, msg


def test_partition_not_read_without_halo(L):
    """halo = 0 is the one-GPU entry: the other partition fields are not looked at -- the call passes every check and
    would launch, so only its refusals are comparable here: the same as with part = NULL."""
    for part in ((5, 99, 0, 3, 4, 7), None):
        rc, untouched = _call(L, part=part, mode=ADD)
        assert rc == ERR_ARG and untouched and "vectors" in L.mpbp_last_error().decode()


@pytest.mark.parametrize("n", [20725, 46341, 2**31 - 1])
@pytest.mark.parametrize("part", [(0, 1, 1, 0, 0, 0), None])
def test_index_overflow_refused(L, n, part):
    """5 n^2 > INT32_MAX (first at n = 20725): MPBP_ERR_OVERFLOW, nothing launched."""
    rc, untouched = _call(L, n=n, part=part, mode=ADD, z=True)
    assert rc == ERR_OVERFLOW and untouched
    msg = L.mpbp_last_error().decode()
    assert msg.startswith("stokes_apply") and "too large" in msg, msg


def test_ext_layout_overflow_refused(L):
    """The whole grid on one rank with ghost rows: 5 n^2 fits at n = 20724, 5 (n + 2) n does not."""
    n = 20724
    assert 5 * n * n <= 2**31 - 1 < 5 * (n + 2) * n
    rc, untouched = _call(L, n=n, part=(0, n, 1, 0, 0, 0))
    assert rc == ERR_OVERFLOW and untouched
    assert L.mpbp_last_error().decode().startswith("stokes_apply_part")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [STORE, ADD, RESID, FAST | STORE, FAST | RESID])
def test_no_partition_is_stokes_apply(L, mode):
    """part = NULL and halo = 0 (its other fields arbitrary) give mpbp_stokes_apply's bits at n = 17."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd._lib import check, ptr, stream_handle
    n = 17
    bp = mp.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
    op = bp.stokes_operator(c=1.0, d_u=-1.0)
    rng = np.random.default_rng(17)
    x, z = (torch.from_numpy(rng.standard_normal(5 * n * n)).cuda() for _ in range(2))
    want = torch.full_like(x, SENTINEL)
    check(L.mpbp_stokes_apply(ctypes.byref(op.prm), ptr(op.cell), ptr(op.uface), ptr(op.vface), mode, ptr(x), ptr(z),
                              ptr(want), stream_handle()))
    for part in (None, _lib.RowPart(0, n, 0, 0, 0, 0), _lib.RowPart(5, 99, 0, 3, 4, 7)):
        got = torch.full_like(x, SENTINEL)
        check(L.mpbp_stokes_apply_part(ctypes.byref(op.prm), ptr(op.cell), ptr(op.uface), ptr(op.vface),
                                       ctypes.byref(part) if part is not None else None, mode, ptr(x), ptr(z),
                                       ptr(got), stream_handle()))
        assert torch.equal(got, want)
    assert not bool((want == SENTINEL).any())
