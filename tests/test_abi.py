"""CPU checks of the C-ABI library: it loads, exports every symbol include/mpbp.h declares, and its
host-only entry points (row-block planner, Chebyshev coefficients, operator sizes) agree with the
oracle.  No compute kernels are launched (there is no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _header_symbols():
    with open(os.path.join(ROOT, "include", "mpbp.h")) as f:
        src = f.read()
    return sorted(set(re.findall(r"\b(mpbp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_header_symbol():
    from mp_block_preconditioners_amd import _lib
    L = _lib.lib()
    declared = _header_symbols()
    assert len(declared) >= 25
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert set(declared) == set(_lib.exported_symbols())
    assert L.mpbp_version().decode().startswith("libmpbp")


def test_library_is_gfx950_code_object():
    from mp_block_preconditioners_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"gfx950" in blob


def test_operator_sizes():
    from mp_block_preconditioners_amd import _lib
    L = _lib.lib()
    n = 7
    N = n * n
    expect = {_lib.OP_A: (5 * N, 5 * N), _lib.OP_F: (4 * N, 4 * N), _lib.OP_D: (N, 4 * N),
              _lib.OP_G: (4 * N, N), _lib.OP_L_N: (2 * N, 2 * N), _lib.OP_D_S: (N, 2 * N),
              _lib.OP_G_N: (2 * N, N), _lib.OP_XI_S: (2 * N, 2 * N)}
    for op, (r, c) in expect.items():
        assert L.mpbp_stokes_rows(n, op) == r
        assert L.mpbp_stokes_cols(n, op) == c
    assert L.mpbp_stokes_rows(n, 99) < 0
    assert b"unknown operator" in L.mpbp_last_error()


def _py_plan(rp, a, b, max_rows=256, cap=4095):
    out = []
    r = a
    while r < b:
        s = e = r
        while e < b and e - s < max_rows and rp[e + 1] - rp[s] <= cap:
            e += 1
        if e == s:
            e = s + 1
        out.append((s, e))
        r = e
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_block_planner(seed):
    from mp_block_preconditioners_amd import _lib
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 40, size=3000)
    lengths[rng.integers(0, 3000, size=3)] = 5000          # rows longer than the LDS stage
    rp = np.zeros(lengths.size + 1, dtype=np.int32)
    np.cumsum(lengths, out=rp[1:])
    L = _lib.lib()
    for a, b in ((0, 3000), (17, 2900), (5, 5)):
        need = L.mpbp_plan_row_blocks(rp.ctypes.data_as(ctypes.c_void_p), a, b, None, 0)
        buf = np.zeros(2 * max(need, 1), dtype=np.int32)
        L.mpbp_plan_row_blocks(rp.ctypes.data_as(ctypes.c_void_p), a, b, buf.ctypes.data_as(ctypes.c_void_p), need)
        got = [tuple(p) for p in buf[: 2 * need].reshape(-1, 2)]
        assert got == _py_plan(rp, a, b)
        for s, e in got:
            assert e - s <= 256 and (rp[e] - rp[s] <= 4095 or e - s == 1)


def test_cheb_coeffs_match_oracle():
    from mp_block_preconditioners_amd import _lib
    from oracle.schur_oracle import cheb_coeffs
    L = _lib.lib()
    for lmin, lmax, k in ((0.05, 2.0, 8), (1e-3, 1.7, 3), (0.0, 1.0, 1)):
        c1 = np.zeros(k)
        c2 = np.zeros(k)
        assert L.mpbp_cheb_coeffs(lmin, lmax, k, c1.ctypes.data_as(ctypes.c_void_p),
                                  c2.ctypes.data_as(ctypes.c_void_p)) == 0
        o1, o2 = cheb_coeffs(lmin, lmax, k)
        assert np.array_equal(c1, o1) and np.array_equal(c2, o2)
    c = np.zeros(2)
    assert L.mpbp_cheb_coeffs(1.0, 1.0, 2, c.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p)) < 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mp_block_preconditioners_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libmpbp.so"))
    with pytest.raises(_lib.MpbpError, match="no CPU fallback"):
        _lib.lib()


def test_wave_table_flags():
    """The row blocks' wave table (csr.wave_table, mpbp_rowblocks.table) on the host: wave entry ranges from row_ptr, and
    the uniform flag exactly for the 64-row waves of 8 / 10 / 12 entries each from an even offset."""
    import numpy as np
    from mp_block_preconditioners_amd.csr import wave_table
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 20, size=1000)
    lens[0:64] = 12          # uniform wave, even start
    lens[64:128] = 10
    lens[128:192] = 7        # uniform but not 8 / 10 / 12
    lens[256:320] = 8
    lens[300] = 9            # broken
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pairs = np.array([[0, 256], [256, 512], [512, 700], [700, 1000]], dtype=np.int32)
    t = wave_table(rp, pairs).reshape(-1, 8)
    assert np.array_equal(t[:, 0], pairs[:, 0]) and np.array_equal(t[:, 1], pairs[:, 1])
    for b, (ra, rb) in enumerate(pairs):
        for w in range(5):
            assert t[b, 2 + w] == rp[min(ra + 64 * w, rb)]
        for w in range(4):
            a = ra + 64 * w
            L = lens[a:a + 64]
            want = int(L[0]) if (rb - a >= 64 and np.all(L == L[0]) and L[0] in (8, 10, 12) and rp[a] % 2 == 0) else 0
            assert (int(t[b, 7]) >> (8 * w)) & 255 == want, (b, w)
    assert (int(t[0, 7]) & 255) == 12 and ((int(t[0, 7]) >> 8) & 255) == (10 if rp[64] % 2 == 0 else 0)


def test_kernel_options_block_lifetime_and_reentry():
    """kernel_options (host-only, mpbp_kernel_opts_set_thread): the installed struct stays referenced while the block is
    active -- the C thread-local pointer refers to it -- and a second entry of the same instance is refused, so the
    previous choice can always be restored."""
    from mp_block_preconditioners_amd import _lib
    base = _lib.kernel_opts()
    ko = _lib.kernel_options(march_rows=7)
    with ko as o:
        assert any(x is o for x in _lib._INSTALLED)
        assert _lib.kernel_opts().march_rows == 7
        with pytest.raises(RuntimeError):
            ko.__enter__()
        with _lib.kernel_options(march_rows=3):
            assert _lib.kernel_opts().march_rows == 3
        assert _lib.kernel_opts().march_rows == 7
    assert not any(x is o for x in _lib._INSTALLED)
    assert _lib.kernel_opts().march_rows == base.march_rows


_MIRRORS = {"mpbp_csr": "Csr", "mpbp_rowblocks": "RowBlocks", "mpbp_sell": "Sell", "mpbp_svl": "Svl",
            "mpbp_row_part": "RowPart", "mpbp_stokes_params": "StokesParams", "mpbp_inner_solver": "InnerSolverC",
            "mpbp_mg_level": "MgLevel", "mpbp_mg": "Mg", "mpbp_schur_plan": "SchurPlan",
            "mpbp_kernel_opts": "KernelOpts"}


def test_ctypes_mirrors_match_the_header(tmp_path):
    """Every ctypes Structure of _lib.py against its struct in include/mpbp.h, as the C compiler lays it out: a C
    program written from the Structures' _fields_ prints sizeof of each struct and offsetof of every field, and each
    value equals ctypes.sizeof / the field's .offset.  A field named differently on the two sides does not compile,
    which fails the test with the compiler's message (it names the field)."""
    from mp_block_preconditioners_amd import _lib
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler found (CC, cc, gcc, clang)"
    expect, prints = [], []
    for cname, pyname in _MIRRORS.items():
        S = getattr(_lib, pyname)
        expect.append((f"sizeof {cname}", ctypes.sizeof(S)))
        prints.append(f'    printf("%zu\\n", sizeof({cname}));')
        for fname, *_ in S._fields_:
            expect.append((f"{cname}.{fname}", getattr(S, fname).offset))
            prints.append(f'    printf("%zu\\n", offsetof({cname}, {fname}));   /* {cname}.{fname} */')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mpbp.h"\nint main(void) {\n'
                   + "\n".join(prints) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, env={**os.environ, "LC_ALL": "C"})   # plain quotes in messages
    if r.returncode != 0:
        named = sorted(set(re.findall(r"no member named ['\u2018](\w+)['\u2019]", r.stderr)))
        pytest.fail(f"_lib.py names fields that include/mpbp.h does not have: {named}\n{r.stderr}")
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(expect)
    wrong = [(what, c, py) for (what, py), c in zip(expect, got) if c != py]
    assert not wrong, f"(what, C, ctypes): {wrong}"


# field: (default, lowest accepted, highest accepted), typed in from the library's source as it stood before the options
# table existed (the positional g_defaults and check_opts' hand-listed chains); not read from the library
_I32_MAX = 2**31 - 1
_OPTS = {
    "march_rows": (0, 0, 4096), "init_diag": (1, 0, 1), "f_pair": (1, 0, 1), "f_direct": (0, 0, 1),
    "gtg_fused": (1, 0, 1), "gtg_tpb": (512, 256, 512), "gtg_drhs": (1, 0, 1), "q13_sym": (1, 0, 1),
    "f_tile": (1, 0, 1), "f_solve": (1, 0, 1), "mg_galerkin_mf": (2, 0, 2), "mg_galerkin_mf_p": (1, 0, 1),
    "pg_direct": (1, 0, 1), "mg_group_rows": (65536, 0, _I32_MAX), "mg_svl": (1, 0, 1), "mg_mf_transfer": (1, 0, 1),
    "csr_table": (1, 0, 1), "mg_fuse_l0": (1, 0, 1), "mg_coarse_tree": (0, 0, 1), "f_solve_tile": (1, 0, 1),
    "q13_mf": (0, 0, 1), "mg_fuse_small": (1, 0, 1), "gtg_solve_tile": (1, 0, 1),
}
# the sixteen setters: those that store any value in their field's range, and those that store value != 0
_RANGE_SETTERS = ("march_rows", "init_diag", "f_pair", "f_direct", "gtg_drhs", "q13_sym", "f_tile", "f_solve",
                  "mg_galerkin_mf", "mg_galerkin_mf_p", "mg_group_rows")
_NORMALISING_SETTERS = ("csr_table", "mg_mf_transfer", "mg_svl", "pg_direct")


def _opts_dict(o):
    return {f: getattr(o, f) for f in _OPTS}


def test_kernel_options_defaults_bounds_and_setters():
    """The kernel options' observable behaviour (host-only): the process defaults, what mpbp_kernel_opts_set_thread
    accepts per field (each bound, and not bound -+ 1; gtg_tpb only 256 and 512), and what each mpbp_set_* accepts,
    stores and refuses, read back through kernel_opts().  mg_group_rows has no upper bound below INT32_MAX, so there
    is no value above it to refuse."""
    from mp_block_preconditioners_amd import _lib
    L = _lib.lib()
    defaults = {f: d for f, (d, _, _) in _OPTS.items()}
    assert [f for f, _ in _lib.KernelOpts._fields_] == list(_OPTS) + ["reserved"]
    assert _opts_dict(_lib.kernel_opts()) == defaults

    def thread_accepts(field, value):
        o = _lib.kernel_opts()
        setattr(o, field, value)
        prev = ctypes.c_void_p()
        rc = L.mpbp_kernel_opts_set_thread(ctypes.byref(o), ctypes.byref(prev))
        if rc == _lib.OK:
            try:
                assert getattr(_lib.kernel_opts(), field) == value
            finally:
                assert L.mpbp_kernel_opts_set_thread(prev, None) == _lib.OK
        else:
            assert rc == _lib.ERR_ARG and b"kernel options out of range" in L.mpbp_last_error()
        return rc == _lib.OK

    for field, (_, lo, hi) in _OPTS.items():
        assert thread_accepts(field, lo) and thread_accepts(field, hi), field
        assert not thread_accepts(field, lo - 1), field
        if hi < _I32_MAX:
            assert not thread_accepts(field, hi + 1), field
    for v in (0, 1, 255, 257, 384, 511, 1024):
        assert not thread_accepts("gtg_tpb", v), v
    assert _opts_dict(_lib.kernel_opts()) == defaults

    def restore():
        for f in _RANGE_SETTERS + _NORMALISING_SETTERS:
            assert getattr(L, "mpbp_set_" + f)(defaults[f]) == _lib.OK
        assert L.mpbp_set_gtg_fused(defaults["gtg_tpb"]) == _lib.OK   # gtg_fused = 1 with the default lanes

    try:
        for f in _RANGE_SETTERS:
            lo, hi = _OPTS[f][1:]
            setter = getattr(L, "mpbp_set_" + f)
            accepted = {lo, hi, (lo + hi) // 2}
            refused = {lo - 1, -_I32_MAX - 1} | ({hi + 1, _I32_MAX} if hi < _I32_MAX else set())
            for v in sorted(accepted):
                assert setter(v) == _lib.OK, (f, v)
                assert _opts_dict(_lib.kernel_opts()) == {**defaults, f: v}, (f, v)
            for v in sorted(refused):
                before = _opts_dict(_lib.kernel_opts())
                assert setter(v) == _lib.ERR_ARG and L.mpbp_last_error(), (f, v)
                assert _opts_dict(_lib.kernel_opts()) == before, (f, v)
            assert setter(defaults[f]) == _lib.OK
        for f in _NORMALISING_SETTERS:
            setter = getattr(L, "mpbp_set_" + f)
            for v, stored in ((0, 0), (1, 1), (2, 1), (-1, 1), (512, 1), (-_I32_MAX - 1, 1), (0, 0), (_I32_MAX, 1)):
                assert setter(v) == _lib.OK, (f, v)
                assert _opts_dict(_lib.kernel_opts()) == {**defaults, f: stored}, (f, v)
            assert setter(defaults[f]) == _lib.OK
        # mpbp_set_gtg_fused: 0 / 1 switch the fused solves and leave the lanes; 256 / 512 switch them on with those lanes
        for v, fused, tpb in ((0, 0, 512), (256, 1, 256), (0, 0, 256), (1, 1, 256), (512, 1, 512), (1, 1, 512)):
            assert L.mpbp_set_gtg_fused(v) == _lib.OK, v
            assert _opts_dict(_lib.kernel_opts()) == {**defaults, "gtg_fused": fused, "gtg_tpb": tpb}, v
        for v in (-1, 2, 255, 257, 511, 513, 1024, _I32_MAX):
            assert L.mpbp_set_gtg_fused(v) == _lib.ERR_ARG, v
            assert _opts_dict(_lib.kernel_opts()) == defaults, v
    finally:
        restore()
    assert _opts_dict(_lib.kernel_opts()) == defaults


def test_every_fragment_is_included_exactly_once():
    """csrc/mpbp.hip is the one translation unit and the csrc/*.inc fragments are its text: every fragment is included
    exactly once, by mpbp.hip alone, and mpbp.hip includes nothing from csrc that is not there.  A text check."""
    csrc = os.path.join(ROOT, "mp-block-preconditioners_amd", "csrc")
    fragments = sorted(f for f in os.listdir(csrc) if f.endswith(".inc"))
    assert fragments
    quoted = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)
    with open(os.path.join(csrc, "mpbp.hip")) as f:
        included = [i for i in quoted.findall(f.read()) if i != "mpbp.h"]   # mpbp.h: include/, found by -I
    assert sorted(included) == fragments, (sorted(set(fragments) - set(included)), sorted(set(included) - set(fragments)),
                                           sorted(i for i in set(included) if included.count(i) > 1))
    for name in fragments:   # no fragment pulls in another: the order is mpbp.hip's alone
        with open(os.path.join(csrc, name)) as f:
            assert not quoted.findall(f.read()), name
