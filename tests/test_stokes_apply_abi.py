"""mpbp_stokes_apply on a machine without a GPU: the header declares it, the library exports it, and every refusal
comes back as its error code with a message in mpbp_last_error() -- the checks run before any HIP call, so nothing is
launched (the vectors here are host arrays that are never dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG, ERR_OVERFLOW = -1, -3
STORE, ADD, RESID, FAST = 0, 1, 2, 0x100


@pytest.fixture(scope="module")
def L():
    from mp_block_preconditioners_amd import _lib
    return _lib.lib()


def test_declared_and_exported(L):
    from mp_block_preconditioners_amd import _lib
    with open(os.path.join(ROOT, "include", "mpbp.h")) as f:
        src = f.read()
    assert re.search(r"\bint\s+mpbp_stokes_apply\s*\(\s*const\s+mpbp_stokes_params\s*\*", src)
    assert "mpbp_stokes_apply" in _lib.exported_symbols()
    fn = getattr(L, "mpbp_stokes_apply")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9


def _call(L, n=8, mode=STORE, prm=True, cell=True, uface=True, vface=True, x=True, z=None, y=True, alias=False):
    from mp_block_preconditioners_amd import _lib
    p = _lib.StokesParams(n, 1.0, 100.0, 1.0, 1.0, -1.0, 1.0, -1.0)
    buf = [np.zeros(8) for _ in range(6)]
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) for b in buf]
    pick = lambda on, q: q if on else None
    return L.mpbp_stokes_apply(ctypes.byref(p) if prm else None, pick(cell, ptrs[0]), pick(uface, ptrs[1]),
                               pick(vface, ptrs[2]), mode, pick(x, ptrs[3]), pick(z, ptrs[4]),
                               ptrs[3] if alias else pick(y, ptrs[5]), None)


@pytest.mark.parametrize("kw,word", [
    (dict(prm=False), "parameters"), (dict(cell=False), "tables"), (dict(uface=False), "tables"),
    (dict(vface=False), "tables"), (dict(x=False), "vectors"), (dict(y=False), "vectors"),
    (dict(alias=True), "vectors"), (dict(alias=True, mode=FAST), "vectors"),
    (dict(mode=ADD), "vectors"), (dict(mode=RESID), "vectors"), (dict(mode=ADD | FAST), "vectors"),
    (dict(n=2), "n >= 3"), (dict(n=0), "n >= 3"), (dict(n=-4), "n >= 3"), (dict(n=2, mode=FAST), "n >= 3"),
    (dict(mode=3), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(mode=FAST | 7), "unknown mode"),
    (dict(mode=0x200), "unknown mode"),
], ids=lambda v: "-".join(f"{k}{w}" for k, w in v.items()) if isinstance(v, dict) else None)
def test_argument_refusals(L, kw, word):
    assert _call(L, **kw) == ERR_ARG
    msg = L.mpbp_last_error().decode()
    assert msg.startswith("stokes_apply") and word in msg, msg


@pytest.mark.parametrize("n", [20725, 46341, 2**31 - 1])
@pytest.mark.parametrize("mode", [STORE, ADD, FAST | RESID])
def test_index_overflow_refused(L, n, mode):
    """5 n^2 > INT32_MAX (first at n = 20725): MPBP_ERR_OVERFLOW, nothing launched."""
    assert 5 * n * n > 2**31 - 1 and 5 * 20724**2 <= 2**31 - 1
    assert _call(L, n=n, mode=mode, z=True) == ERR_OVERFLOW
    msg = L.mpbp_last_error().decode()
    assert msg.startswith("stokes_apply") and "too large" in msg, msg
