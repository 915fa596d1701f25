"""Geometric multigrid for the inner inverses F^-1 and Gt_G^-1 of the approximate Schur preconditioner.

The reference approximates both inverses with ILUT (solve.py:250-254) and names the scalable choice in
its own comments: "In IBAMR, we'd use Multigrid PC with Jacobi smoother" (solve.py:266, 274).  This is
that choice on the GPU:

* levels: the periodic n x n MAC grid coarsened by 2 per direction down to n <= ``coarsest`` (at least once;
  odd n stops -- or, with ``coarsen="any"``, coarsens to n // 2 by interpolated transfers, so any n >= 5 works);
* transfers: per field, linear interpolation along each axis -- cell-centred (p; u along y; v along x)
  or node-centred (u along x, v along y) -- as CSR P, and R = P^T (``mpbp_mg_transfer_*``, exact values);
* coarse operators: Galerkin A_{l+1} = R (A_l P) with the library's SpGEMM (every product kept);
* smoother: Chebyshev-Jacobi on [lmax / ratio, lmax] with lmax the Gershgorin bound of diag(A)^-1 A (the default,
  ``smoother="point"``); or, for the four velocity fields, ``smoother="coupled"``: Chebyshev on B^-1 A with B the 2 x 2
  blocks that couple the two phases at each face (point-block Jacobi), lmax = ||B^-1 A||_inf -- robust at large drag,
  where point Jacobi stops smoothing;
* coarsest level: its dense pseudo-inverse (computed once on the host), applied by a dense kernel (one row per
  lane, the CSR row's order) from a column-major copy;
* layouts: every level's operator and transfers also get a SELL-64 copy when their rows fit (< 256 entries):
  the Galerkin coarse operators' long uniform rows (20-50 entries) stream at HBM speed one row per lane, where
  the CSR kernel's per-wave chunks serve rows of <= 12 entries (same bits either way).

``Multigrid.solve`` runs ``cycles`` V-cycles from x = 0 through ``mpbp_mg_solve`` (graph-capturable).
Inside ``ApproxSchurPreconditioner`` (``InnerSolver("mg", cycles)``) level 0 is the apply's own F / Gt_G
operator -- matrix-free when the plan is -- with the same bits.  oracle/mg_oracle.py restates the cycle.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_handle
from .csr import DeviceCSR, DeviceSELL, csr_from_row_nnz, spgemm, timed_phase

CELL, NODE = _lib.MG_CELL, _lib.MG_NODE
# (row axis, column axis) kinds of [u_n, v_n, u_s, v_s]: u at (-(r+1/2) dy, c dx), v at (-r dy, (c+1/2) dx)
# (utils.fill_sol_and_RHS_vecs), p at cell centres
FIELDS_VELOCITY = ((CELL, NODE), (NODE, CELL), (CELL, NODE), (NODE, CELL))
FIELDS_PRESSURE = ((CELL, CELL),)


COARSENINGS = ("even", "any")
SMOOTHERS = ("point", "coupled")


def _check_smoother(smoother: str):
    if smoother not in SMOOTHERS:
        raise ValueError(f"smoother must be one of {SMOOTHERS}, not {smoother!r}")


def coupled_tables(A: DeviceCSR, out=None):
    """(cpl_p, cpl_q) of the phase-coupled smoother (mpbp_cpl_blocks): row i's line a' / det, -k / det of the inverse of
    the 2 x 2 block that rows i and i +- nrows / 2 form.  out: the pair of tensors to fill in place.  MpbpError naming
    the first row without a stored diagonal or with a determinant that is not finite and positive."""
    p, q = out if out is not None else (torch.empty(A.shape[0], dtype=torch.float64, device=A.device) for _ in range(2))
    check(lib().mpbp_cpl_blocks(ctypes.byref(A.cstruct()), ptr(p), ptr(q), stream_handle()))
    return p, q


def coupled_bound(A: DeviceCSR, p: torch.Tensor, q: torch.Tensor) -> float:
    """||B^-1 A||_inf with B the 2 x 2 phase blocks of coupled_tables (mpbp_cpl_bound): the coupled smoother's lmax."""
    out = ctypes.c_double(0.0)
    check(lib().mpbp_cpl_bound(ctypes.byref(A.cstruct()), ptr(p), ptr(q), ctypes.byref(out), stream_handle()))
    return out.value


def _check_coarsen(coarsen: str):
    if coarsen not in COARSENINGS:
        raise ValueError(f"coarsen must be one of {COARSENINGS}, not {coarsen!r}")


def transfer(n: int, fields, which: int, device, coarsen: str = "even") -> DeviceCSR:
    """P (which = MG_P: fine x coarse) or R = P^T (MG_R) of the n x n grid, built on the GPU.  coarsen="even": n even,
    the 2:1 lists; "any": n >= 5 of either parity coarsened to n // 2, each fine point interpolated linearly from its
    two coarse neighbours (mpbp_mg_transfer_any_*; for even n the same matrix bit for bit)."""
    _check_coarsen(coarsen)
    count, fill = ((lib().mpbp_mg_transfer_any_count, lib().mpbp_mg_transfer_any_fill) if coarsen == "any" else
                   (lib().mpbp_mg_transfer_count, lib().mpbp_mg_transfer_fill))
    kinds = np.ascontiguousarray(np.asarray(fields, dtype=np.int32).reshape(-1))
    nf = len(fields)
    rows = nf * (n * n if which == _lib.MG_P else (n // 2) ** 2)
    cols = nf * ((n // 2) ** 2 if which == _lib.MG_P else n * n)
    row_nnz = torch.empty(max(rows, 1), dtype=torch.int32, device=device)[:rows]
    check(count(n, nf, kinds.ctypes.data_as(ctypes.c_void_p), which, ptr(row_nnz), stream_handle()))
    rp, ci, va = csr_from_row_nnz(row_nnz, (rows, cols), device)
    check(fill(n, nf, kinds.ctypes.data_as(ctypes.c_void_p), which, ptr(rp), ptr(ci), ptr(va), stream_handle()))
    return DeviceCSR(rp, ci, va, (rows, cols))


def transfer_rows(n: int, fields, which: int, rows: torch.Tensor) -> DeviceCSR:
    """Rows `rows` (device int32 global ids) of transfer(n, fields, which) with their global columns, the same entries
    (mpbp_mg_transfer_rows_*): a rank's band of a row-partitioned hierarchy."""
    kinds = np.ascontiguousarray(np.asarray(fields, dtype=np.int32).reshape(-1))
    nf = len(fields)
    cols = nf * ((n // 2) ** 2 if which == _lib.MG_P else n * n)
    rows = rows.to(torch.int32).contiguous()
    m = rows.numel()
    nrows = nf * (n * n if which == _lib.MG_P else (n // 2) ** 2)
    if m and (int(rows.min()) < 0 or int(rows.max()) >= nrows):   # the kernel derives (field, row, column) from the id
        raise ValueError(f"transfer_rows: row ids must lie in [0, {nrows}) for {nf} fields of the {n}^2 level")
    row_nnz = torch.empty(max(m, 1), dtype=torch.int32, device=rows.device)[:m]
    check(lib().mpbp_mg_transfer_rows_count(n, nf, kinds.ctypes.data_as(ctypes.c_void_p), which, ptr(rows), m,
                                            ptr(row_nnz), stream_handle()))
    rp, ci, va = csr_from_row_nnz(row_nnz, (m, cols), rows.device)
    check(lib().mpbp_mg_transfer_rows_fill(n, nf, kinds.ctypes.data_as(ctypes.c_void_p), which, ptr(rows), m, ptr(rp),
                                           ptr(ci), ptr(va), stream_handle()))
    return DeviceCSR(rp, ci, va, (m, cols))


def sell_copy(A: DeviceCSR) -> DeviceSELL | None:
    """SELL-64 copy of A when every row has < 256 entries (the layout's row-length byte), else None."""
    rp = A.row_ptr_host
    if A.shape[0] == 0 or int(np.max(np.diff(rp))) > 255:
        return None
    return A.to_sell()


class StencilValues:
    """Stencil-values layout (``mpbp_svl``) of a translation-invariant operator on nf stacked m x m periodic fields: every
    row of field f holds the same K (field, dr, dc) offsets, so only the values are kept, slot-major, and the kernel
    rebuilds an interior row's columns as row + delta[f][s].  Built on the GPU from the CSR arrays (``build``), which it
    verifies: uniform row length, every row's wrapped offsets a permutation of the field's K slots, interior rows in
    slot order (so the interior sums are the CSR row's, bit for bit).  Rows within `reach` of the periodic edge are
    listed for the kernel's CSR path.  None when the operator is not of that form."""

    def __init__(self, A: DeviceCSR, nf: int, m: int, reach: int, K: int, delta, vals, edge_rows, gather=None):
        self.A, self.nf, self.m, self.reach, self.slots = A, nf, m, reach, K
        self.delta, self.vals, self.edge_rows = delta, vals, edge_rows
        self.gather = gather   # int32: vals[i] = A.val[gather[i]], the slot permutation build() found (refill)
        self._cs = _lib.Svl(nf, m, reach, K, delta.data_ptr(), vals.data_ptr(),
                            edge_rows.data_ptr() if edge_rows.numel() else None, int(edge_rows.numel()), 0)

    def cstruct(self):
        return self._cs

    @classmethod
    def build(cls, A: DeviceCSR, nf: int, m: int) -> "StencilValues | None":
        if A.shape != (nf * m * m, nf * m * m) or A.nnz == 0:
            return None
        arrays = _stencil_values_arrays(A.row_ptr, A.col_idx, A.val, nf, m)
        return None if arrays is None else cls(A, nf, m, *arrays)

    def refill(self):
        """The operator's current values scattered into the existing slot-major array by the permutation found at build
        time (the pattern is the build's: nothing is verified again, nothing allocated)."""
        if self.gather is None:
            raise ValueError("this StencilValues was not made by build(): it has no slot permutation to refill by")
        torch.index_select(self.A.val, 0, self.gather, out=self.vals)

    def matvec(self, x: torch.Tensor, out: torch.Tensor | None = None, mode=_lib.SPMV_STORE,
               z: torch.Tensor | None = None) -> torch.Tensor:
        if out is None:
            out = torch.empty(self.A.shape[0], dtype=torch.float64, device=self.A.device)
        check(lib().mpbp_svl_spmv(ctypes.byref(self._cs), ctypes.byref(self.A.cstruct()), mode, ptr(x), ptr(z),
                                  ptr(out), stream_handle()))
        return out


def stencil_values_arrays(row_ptr: torch.Tensor, col_idx: torch.Tensor, val: torch.Tensor, nf: int, m: int):
    """(reach, K, delta[nf * K], vals[K * N] slot-major, edge_rows) of StencilValues from CSR arrays (any torch device),
    or None when the operator is not translation-invariant in that sense (see StencilValues)."""
    arrays = _stencil_values_arrays(row_ptr, col_idx, val, nf, m)
    return None if arrays is None else arrays[:5]


def _stencil_values_arrays(row_ptr: torch.Tensor, col_idx: torch.Tensor, val: torch.Tensor, nf: int, m: int):
    """stencil_values_arrays' tuple and the int32 entry index `gather` with vals[i] = val[gather[i]]."""
    N = nf * m * m
    if row_ptr.numel() != N + 1 or m < 4:
        return None
    dev = row_ptr.device
    rp = row_ptr.long()
    lens = rp[1:] - rp[:-1]
    K = int(lens[0])
    if K < 1 or nf * K > 256 or not bool(torch.all(lens == K)):
        return None
    e = torch.arange(col_idx.numel(), device=dev)
    rows, pos = e // K, e % K
    del e
    mm = m * m
    ci = col_idx.long()
    f, cell = rows // mm, rows % mm
    r, c = cell // m, cell % m
    fc, cc = ci // mm, ci % mm
    dr = (cc // m - r + m // 2) % m - m // 2
    dc = (cc % m - c + m // 2) % m - m // 2
    del cell, cc
    R = int(torch.maximum(dr.abs().max(), dc.abs().max()))
    if m % 2 or m < 2 * R + 4 or K * N > 2 ** 31 - 1:
        return None
    w = 2 * R + 1
    table = torch.full((nf, nf, w, w), -1, dtype=torch.long, device=dev)
    delta = torch.empty(nf, K, dtype=torch.int32, device=dev)
    for f0 in range(nf):
        base = f0 * mm + (m // 2) * m + m // 2
        sl = slice(base * K, base * K + K)
        table[f0, fc[sl], dr[sl] + R, dc[sl] + R] = torch.arange(K, device=dev)
        delta[f0] = (ci[sl] - base).to(torch.int32)
    slot = table[f, fc, dr + R, dc + R]
    del fc, dr, dc, table
    if bool((slot < 0).any()):
        return None
    seen = torch.bincount(rows * K + slot, minlength=N * K)
    if not bool(torch.all(seen == 1)):
        return None
    del seen
    if bool(((slot != pos) & (r >= R) & (r < m - R) & (c >= R) & (c < m - R)).any()):
        return None
    R += R & 1   # the kernel's interior cells go in pairs from an even column: an odd reach widens the edge band
    interior = (r >= R) & (r < m - R) & (c >= R) & (c < m - R)
    vals = torch.empty(K * N, dtype=torch.float64, device=dev)
    where = slot * N + rows
    vals[where] = val
    gather = torch.empty(K * N, dtype=torch.int32, device=dev)   # (every slot seen once: `where` is a permutation)
    gather[where] = torch.arange(K * N, dtype=torch.int32, device=dev)
    del where
    row_int = interior.view(N, K)[:, 0]
    edge = torch.nonzero(~row_int).reshape(-1).to(torch.int32)
    return R, K, delta.reshape(-1).contiguous(), vals, edge, gather


def set_transfer_kinds(mg_struct, fields, n0: int):
    """mpbp_mg.tr_*: the transfers' field kinds and level 0's grid size (matrix-free whole-grid transfers)."""
    mg_struct.tr_nfields = len(fields)
    mg_struct.tr_n0 = int(n0)
    for f, (ky, kx) in enumerate(fields):
        mg_struct.tr_ky[f] = ky
        mg_struct.tr_kx[f] = kx


SVL_MIN_ROWS = 65536     # Multigrid's default: levels >= 1 above this many rows get a stencil-values copy
MAX_COARSE_ROWS = 8192   # the coarsest level's dense pseudo-inverse: 8192^2 doubles = 512 MB, an O(m^3) host pinv
# Singular values below COARSE_RCOND * sigma_max of the coarsest operator are its null space.  Gt_G on the periodic
# grid annihilates constants; after six Galerkin products that mode's singular value is roundoff, 8.5e-16 sigma_max at
# 256^2 but 5.6e-15 at 1024^2 -- above numpy's default cut (1e-15), so the pseudo-inverse inverted it and the pressure
# solve's output carried a ~1e17 constant.  The next singular values are 9e-2 (Gt_G) and, for F, 7.5e-6 (eta ratio
# 100) / 7.5e-8 (10^4) (tools/coarse_spectrum.py): 1e-11 sits orders of magnitude from both.
COARSE_RCOND = 1e-11
# Chebyshev acceleration (accel="chebyshev"): the interval's rho = ACCEL_RHO_MARGIN x the largest of the power iteration's
# last three ratios (Multigrid.contraction).  The ratios still climb after 8 steps (0.037 -> 0.090 for F at 64^2), so the
# estimate sits below the spectral radius; the margin covers part of that and the iteration tolerates the rest (an
# eigenvalue just outside the interval is still damped), while rho = 0.15 there already loses the gain.
ACCEL_RHO_MARGIN = 1.1
ACCEL_RHO_MAX = 0.5      # an estimate at or above this: a singular operator (E keeps its null space) or no contraction
ACCELS = (None, "chebyshev")


def _dense_inverse_host(A: DeviceCSR) -> np.ndarray:
    """The pseudo-inverse dense_inverse_csr stores, on the host (row-major)."""
    Ad = A.to_scipy().toarray()
    return np.ascontiguousarray(np.linalg.pinv(Ad, rcond=COARSE_RCOND))


def dense_inverse_csr(A: DeviceCSR) -> tuple[DeviceCSR, np.ndarray]:
    """The pseudo-inverse of a small operator as a CSR with every entry stored (rows of ncols entries)."""
    if A.shape[0] > MAX_COARSE_ROWS:
        raise ValueError(f"coarsest level has {A.shape[0]} rows (> {MAX_COARSE_ROWS}): its dense pseudo-inverse would "
                         f"need {A.shape[0] ** 2 * 8 / 1e9:.1f} GB and an O(m^3) factorisation; coarsening stops at an odd "
                         "grid size, so use a grid n = m 2^k with a small m (or a larger `coarsest`)")
    inv = _dense_inverse_host(A)
    m = inv.shape[0]
    dev = A.device
    rp = np.arange(0, m * m + 1, m, dtype=np.int32)
    ci = np.tile(np.arange(m, dtype=np.int32), m)
    M = DeviceCSR(torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev),
                  torch.from_numpy(inv.reshape(-1).copy()).to(dev), (m, m), row_ptr_host=rp)
    return M, inv


def _stop_coarsening(m: int, coarsest: int, nlevels: int, coarsen: str) -> bool:
    """Whether size m is the hierarchy's last level when nlevels levels exist (at least one coarsening)."""
    if m <= coarsest and nlevels > 1:
        return True
    return m < 5 if coarsen == "any" else bool(m % 2 or m // 2 < 2)


def level_sizes(n: int, coarsest: int, coarsen: str = "even") -> list[int]:
    """Grid sizes of the hierarchy, down to <= coarsest (at least one coarsening).  coarsen="even": halve while even;
    "any": halve with floor whatever the parity (an odd level's transfers interpolate, transfer(coarsen="any"))."""
    _check_coarsen(coarsen)
    sizes = [n]
    m = n
    while not _stop_coarsening(m, coarsest, len(sizes), coarsen):
        m //= 2
        sizes.append(m)
    return sizes


class Multigrid:
    """V-cycle hierarchy over a stacked-field operator A (DeviceCSR) of an n x n periodic grid.

    fields   per stacked field, the (row axis, column axis) kinds -- FIELDS_VELOCITY for F, FIELDS_PRESSURE
             for Gt_G
    pre/post Chebyshev-Jacobi smoothing sweeps per level; ratio: lmin = lmax / ratio
    cycles   V-cycles per solve (x0 = 0); coarsest: stop coarsening at n <= coarsest
    sell     SELL-64 copies of the operators / transfers and the dense coarse kernel (False: CSR throughout)
    fine_sell  also a SELL copy of level 0's operator (the standalone solve's fine level)
    svl_min_rows  levels >= 1 with more rows get a stencil-values copy (StencilValues; None: never) -- used where the
             grouped small-level kernel is not (kernel option mg_group_rows)
    kernel_opts  overrides of the process-default kernel choices for this hierarchy's standalone solve (_lib.KernelOpts
             field names)
    accel    None: ``cycles`` stationary V-cycles x <- x + M (b - A x).  "chebyshev": the fixed Chebyshev semi-iteration
             over the same ``cycles`` V-cycles for spec(M A) in [1 - rho, 1] (mpbp_mg_accel_coeffs, mpbp_mg_combine) --
             no inner products, no extra operator apply, still a linear operator.  Needs a symmetric cycle (pre ==
             post) and a nonsingular operator.
    coarsen  "even" (default): halve while the size is even, the first odd size is the coarsest level.  "any": halve with
             floor whatever the parity (n >= 5), an odd level's P / R interpolating each fine point from its two coarse
             neighbours (transfer(coarsen="any")); Galerkin rows below an odd level reach 86 entries, so the products
             and refresh take the wide forms (<= 128).  Odd-derived levels get no stencil-values copy and no fused
             residual-restriction kernel (their rows are ragged); everything else, accel included, is unchanged.
    smoother "point" (default): Chebyshev-Jacobi on diag(A)^-1 A, today's code paths and bits.  "coupled": point-block
             Jacobi over the two phases -- rows i and i + nrows / 2 (u_n, u_s at one face; v_n, v_s likewise) are
             relaxed together through the inverse of their 2 x 2 block (coupled_tables), the interval's lmax is
             ||B^-1 A||_inf (coupled_bound).  Four stacked fields only (FIELDS_VELOCITY); one GPU only.  Each sweep is
             a residual launch and one mpbp_cpl_update launch: none of the fused point-Jacobi launches is taken, so
             at drag xi = 1 (where both smoothers contract alike) it costs more than "point"; it is for xi h^2 >~ eta.
    cpl_fuse smoother="coupled", level 0 the Schur apply's matrix-free F: one launch per sweep (set_coupled_fuse)
    rho      the contraction bound of one V-cycle; None: estimated here (and again by refresh) as ACCEL_RHO_MARGIN x
             the largest of contraction()'s last three ratios -- setup work that synchronises with the host
    """

    def __init__(self, A: DeviceCSR, n: int, fields=FIELDS_PRESSURE, pre: int = 2, post: int = 2, cycles: int = 1,
                 ratio: float = 4.0, coarsest: int = 8, diag: torch.Tensor | None = None, sell: bool = True,
                 fine_sell: bool = True, svl_min_rows: int | None | str = "default", kernel_opts: dict | None = None,
                 accel: str | None = None, rho: float | None = None, coarsen: str = "even",
                 smoother: str = "point", cpl_fuse: bool = True):
        nf = len(fields)
        _check_coarsen(coarsen)
        _check_smoother(smoother)
        if smoother == "coupled" and nf != 4:
            raise ValueError(f'smoother="coupled" pairs the two phases of the four velocity fields (FIELDS_VELOCITY): '
                             f"this hierarchy has {nf} field{'s' if nf != 1 else ''}")
        self.smoother = smoother
        if accel not in ACCELS:
            raise ValueError(f"accel must be one of {ACCELS}, not {accel!r}")
        if accel is not None and pre != post:
            raise ValueError(f"accel={accel!r} needs a symmetric cycle, pre == post (got V({pre},{post})): the "
                             "Chebyshev interval [1 - rho, 1] holds for a symmetric M only")
        if rho is not None and (accel is None or not 0.0 < float(rho) < 1.0):
            raise ValueError("rho needs accel and 0 < rho < 1")
        if A.shape != (nf * n * n, nf * n * n):
            raise ValueError(f"operator {A.shape} is not {nf} fields of a {n} x {n} grid")
        if coarsen == "any":
            if n < 5:
                raise ValueError('multigrid with coarsen="any" needs a grid n >= 5')
        elif n < 4 or n % 2 or n // 2 < 2:
            raise ValueError("multigrid needs an even grid n >= 4")
        if pre < 1 or post < 1 or cycles < 1:
            raise ValueError("pre, post and cycles must be >= 1")
        self.n, self.fields, self.pre, self.post, self.cycles, self.ratio = n, tuple(fields), pre, post, cycles, ratio
        self.coarsest, self.coarsen = coarsest, coarsen
        dev = A.device
        self.device = dev
        sizes = level_sizes(n, coarsest, coarsen)
        if nf * sizes[-1] ** 2 > MAX_COARSE_ROWS:   # refuse before any Galerkin product is formed
            why, hint = (("stopping at `coarsest`", f": lower `coarsest` (now {coarsest})") if coarsen == "any" else
                         ("stopping at an odd size", '; coarsen="any" coarsens odd sizes too'))
            raise ValueError(f"grid {n} coarsens to {sizes} ({why}): the coarsest level's "
                             f"{nf * sizes[-1] ** 2} rows exceed the dense inverse's {MAX_COARSE_ROWS}{hint}")
        wide = coarsen == "any"   # Galerkin rows below an odd level reach 86 entries
        self.ops, self.diags, self.R, self.P, self.bounds, self.sizes = [], [], [], [], [], []
        self.cpl = []   # smoother="coupled": per level (cpl_p, cpl_q), None on the coarsest (it is not smoothed)
        m = n
        while True:
            last = _stop_coarsening(m, coarsest, len(self.ops) + 1, coarsen)
            # (the coupled tables before the diagonal: their error names the row a missing diagonal sits in)
            self.cpl.append(coupled_tables(A) if smoother == "coupled" and not last else None)
            d = diag if (not self.ops and diag is not None) else A.diagonal()
            lmax = coupled_bound(A, *self.cpl[-1]) if self.cpl[-1] is not None else A.gershgorin(d)
            self.ops.append(A)
            self.diags.append(d)
            self.bounds.append((lmax / ratio, lmax))
            self.sizes.append(m)
            if _stop_coarsening(m, coarsest, len(self.ops), coarsen):   # (at least one coarsening)
                break
            rule = "any" if m % 2 else "even"   # (an even level's lists are the same under either rule)
            P = transfer(m, fields, _lib.MG_P, dev, coarsen=rule)
            R = transfer(m, fields, _lib.MG_R, dev, coarsen=rule)
            self.P.append(P)
            self.R.append(R)
            A = spgemm(R, spgemm(A, P, wide=wide), wide=wide)
            m //= 2
        if len(self.ops) < 2:
            raise ValueError(f"grid {n} gives a single level (coarsest={coarsest})")
        self.coarse_inv, self.coarse_inv_host = dense_inverse_csr(self.ops[-1])
        # the dense kernel's column-major copy (None: the CSR form)
        self.coarse_dense = (torch.from_numpy(np.ascontiguousarray(self.coarse_inv_host.T)).to(dev)
                             if sell else None)
        # SELL-64 copies of the operators (level 0 too: the standalone solve's fine level) and transfers
        # (fine_sell=False: level 0's operator is the caller's own -- the Schur apply's matrix-free F / Gt_G)
        self.sells = [[sell_copy(M) if sell and (l > 0 or fine_sell or grp is not self.ops) else None
                       for l, M in enumerate(grp)] for grp in (self.ops, self.R, self.P)]
        # stencil-values copies of the large coarse levels (8 B per entry instead of 12 B; same bits)
        if svl_min_rows == "default":
            svl_min_rows = SVL_MIN_ROWS
        self.svls = [StencilValues.build(M, nf, self.sizes[l])
                     if (l > 0 and svl_min_rows is not None and M.shape[0] > svl_min_rows) else None
                     for l, M in enumerate(self.ops)]
        f64 = dict(dtype=torch.float64, device=dev)
        self.work = [[torch.zeros(M.shape[0], **f64) for _ in range(5)] for M in self.ops]
        self._levels = (_lib.MgLevel * len(self.ops))()
        empty_csr, empty_blk = _lib.Csr(0, 0, 0, None, None, None), _lib.RowBlocks(None, 0)
        for l, M in enumerate(self.ops):
            L = self._levels[l]
            L.nrows, L.pre, L.post = M.shape[0], pre, post
            L.lmin, L.lmax = self.bounds[l]
            L.A, L.A_blocks, L.diag = M.cstruct(), M.blocks.cstruct(), self.diags[l].data_ptr()
            if l < len(self.R):
                L.R, L.R_blocks = self.R[l].cstruct(), self.R[l].blocks.cstruct()
                L.P, L.P_blocks = self.P[l].cstruct(), self.P[l].blocks.cstruct()
            else:
                L.R = L.P = empty_csr
                L.R_blocks = L.P_blocks = empty_blk
            L.x, L.t, L.r, L.d, L.b = (w.data_ptr() for w in self.work[l])
            for name, grp in zip(("A_sell", "R_sell", "P_sell"), self.sells):
                S = grp[l] if l < len(grp) else None
                setattr(L, name, S.cstruct() if S is not None else _lib.Sell(0, 0, 0, 0, None, None, None, None))
            if self.svls[l] is not None:
                L.A_svl = ctypes.pointer(self.svls[l].cstruct())
            if self.cpl[l] is not None:
                L.cpl_p, L.cpl_q = (t.data_ptr() for t in self.cpl[l])
        self._mg = _lib.Mg(len(self.ops), cycles, ctypes.cast(self._levels, ctypes.POINTER(_lib.MgLevel)),
                           self.coarse_inv.cstruct(), self.coarse_inv.blocks.cstruct(),
                           self.coarse_dense.data_ptr() if self.coarse_dense is not None else None)
        # the standalone solve's kernel choices (inside a Schur apply the preconditioner's own govern)
        self.kernel_opts = _lib.kernel_opts(kernel_opts)
        self._mg.opts = ctypes.pointer(self.kernel_opts)
        set_transfer_kinds(self._mg, self.fields, n)
        self._mg.smoother = _lib.MG_SMOOTH_COUPLED if smoother == "coupled" else _lib.MG_SMOOTH_POINT
        self.set_coupled_fuse(cpl_fuse)
        # Chebyshev acceleration: x_k and x_{k-1} (the cycle's own buffers do not keep its initial guess), and rho
        self.accel = accel
        self.rho_estimated = accel is not None and rho is None
        self._rho = None if rho is None else float(rho)
        self.accel_x = None
        if accel is not None:
            self.accel_x = [torch.zeros(self.ops[0].shape[0], **f64) for _ in range(2)]
            for i, t in enumerate(self.accel_x):
                self._mg.accel_x[i] = t.data_ptr()
            if self.rho_estimated:
                self._rho = self.estimate_rho()
            self._mg.accel_rho = self._rho
            self._mg.accel = _lib.MG_ACCEL_CHEBYSHEV

    @property
    def rho(self) -> float | None:
        """The accelerated iteration's contraction bound (None without accel)."""
        return self._rho

    def contraction(self, steps: int = 8, seed: int = 0) -> list[float]:
        """Power iteration on the error propagator E = I - M A of ONE zero-start V-cycle M over the stored level-0
        operator: e_0 = numpy.random.default_rng(seed).standard_normal (host), e_{j+1} = e_j - V(A e_j); returns
        ||e_{j+1}||_2 / ||e_j||_2 per step.  The ratios climb towards E's spectral radius.  Setup work: allocates and
        synchronises with the host."""
        A = self.ops[0]
        e = torch.from_numpy(np.random.default_rng(seed).standard_normal(A.shape[0])).to(self.device)
        saved = (self._mg.cycles, self._mg.accel)
        self._mg.cycles, self._mg.accel = 1, _lib.MG_ACCEL_NONE
        try:
            ratios = []
            norm = float(torch.linalg.vector_norm(e))
            Ae, Ve = torch.empty_like(e), torch.empty_like(e)
            for _ in range(steps):
                A.matvec(e, out=Ae)
                self.solve(Ae, out=Ve)
                e = e - Ve
                new = float(torch.linalg.vector_norm(e))
                ratios.append(new / norm)
                norm = new
        finally:
            self._mg.cycles, self._mg.accel = saved
        return ratios

    def estimate_rho(self) -> float:
        """ACCEL_RHO_MARGIN x the largest of contraction()'s last three ratios; ValueError at ACCEL_RHO_MAX or above."""
        rho = ACCEL_RHO_MARGIN * max(self.contraction()[-3:])
        if not rho < ACCEL_RHO_MAX:
            raise ValueError(f"accel={self.accel!r}: the estimated contraction bound rho = {rho:.3g} is not below "
                             f"{ACCEL_RHO_MAX}: the operator is singular (its null space gives I - M A an eigenvalue of "
                             "1) or the cycle does not contract; use the stationary cycles (accel=None)")
        return rho

    def refresh(self, diag: torch.Tensor | None = None, timings: dict | None = None):
        """New values on the same grid: level 0's operator (the caller's) already holds them.  Recomputes, in place at
        every address the hierarchy's struct holds, each coarser operator (one fused R (A P) launch per level,
        mpbp_triple_refill -- its wide form under coarsen="any" --, no A P intermediate), every level's diagonal and
        smoothing interval (the coupled smoother's tables too), the SELL and stencil-values copies and the coarsest pseudo-inverse -- what a fresh Multigrid over the same operator computes,
        bit for bit, with no structural work.  diag: level 0's new diagonal (default: recomputed; the tensor given to
        the constructor, refreshed by the caller, may be passed again).  timings: seconds per phase, each synchronised.
        An estimated acceleration rho is estimated again (phase "accel_rho"; an explicit one stays).
        Graphs captured before carry the old smoothing intervals (and the acceleration's coefficients) as kernel
        arguments: capture again."""
        triple_refill = lib().mpbp_triple_refill_wide if self.coarsen == "any" else lib().mpbp_triple_refill
        for l, A in enumerate(self.ops):
            if l > 0:
                with timed_phase(timings, "galerkin"):
                    check(triple_refill(ctypes.byref(self.R[l - 1].cstruct()), ctypes.byref(self.ops[l - 1].cstruct()),
                                        ctypes.byref(self.P[l - 1].cstruct()), _lib.ASSOC_RIGHT, 1.0, 1.0,
                                        ctypes.byref(A.cstruct()), stream_handle()))
            with timed_phase(timings, "diag_bounds"):
                d = self.diags[l]
                if l == 0 and diag is not None:
                    if diag.data_ptr() != d.data_ptr():
                        d.copy_(diag)
                else:
                    d.copy_(A.diagonal())
                if self.cpl[l] is not None:   # the coupled tables in place, and their bound
                    coupled_tables(A, out=self.cpl[l])
                    lmax = coupled_bound(A, *self.cpl[l])
                else:
                    lmax = A.gershgorin(d)
                self.bounds[l] = (lmax / self.ratio, lmax)
                self._levels[l].lmin, self._levels[l].lmax = self.bounds[l]
        with timed_phase(timings, "layouts"):
            for S in self.sells[0]:   # the transfers' copies hold geometry only
                if S is not None:
                    S.refill()
            for V in self.svls:
                if V is not None:
                    V.refill()
        with timed_phase(timings, "host_pinv"):
            inv = _dense_inverse_host(self.ops[-1])
            self.coarse_inv_host = inv
            self.coarse_inv.val.copy_(torch.from_numpy(inv.reshape(-1)))
            if self.coarse_dense is not None:
                self.coarse_dense.copy_(torch.from_numpy(np.ascontiguousarray(inv.T)))
        if self.rho_estimated:   # (an explicit rho stays)
            with timed_phase(timings, "accel_rho"):
                self._rho = self.estimate_rho()
                self._mg.accel_rho = self._rho

    def set_coupled_fuse(self, on: bool):
        """smoother="coupled" with level 0 the Schur apply's matrix-free F: each sweep as one launch (on, the default:
        the stencil kernel's cell-wise epilogue; exact numerics give the same bits) or as the residual launch followed
        by mpbp_cpl_update (off).  No effect on a stored level 0 or with the point smoother.  Graphs captured before
        keep their launches: capture again."""
        self.cpl_fuse = bool(on)
        self._mg.cpl_fuse = 1 if (on and self.smoother == "coupled") else 0

    def set_matrix_free_transfers(self, on: bool):
        """Name (on) or hide (off) the field kinds in the hierarchy's struct: with them the whole-grid levels' transfers
        run matrix-free (same bits as the stored P / R)."""
        set_transfer_kinds(self._mg, self.fields if on else (), self.n)

    @property
    def nlevels(self) -> int:
        return len(self.ops)

    def cstruct(self) -> _lib.Mg:
        return self._mg

    def solve(self, b: torch.Tensor, out: torch.Tensor | None = None, sub: torch.Tensor | None = None) -> torch.Tensor:
        """x = MG^-1 b (``cycles`` V-cycles from 0, accelerated when accel is set); sub - x when sub is given."""
        n0 = self.ops[0].shape[0]
        assert b.is_cuda and b.dtype == torch.float64 and b.numel() == n0
        if out is None:
            out = torch.empty(n0, dtype=torch.float64, device=self.device)
        check(lib().mpbp_mg_solve(ctypes.byref(self._mg), ptr(b), ptr(sub), ptr(out), stream_handle()))
        return out

    def __repr__(self):
        return (f"Multigrid(levels={self.sizes}, fields={len(self.fields)}, pre={self.pre}, post={self.post}, "
                f"cycles={self.cycles}, ratio={self.ratio}" + (", coarsen='any'" if self.coarsen == "any" else "")
                + (f", smoother={self.smoother!r}" if self.smoother != "point" else "")
                + (f", accel={self.accel!r}, rho={self._rho:.4g}" if self.accel else "") + ")")
