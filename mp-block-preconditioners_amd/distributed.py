"""Row partition of the MAC grid over ranks (one process per GPU) with halo exchange over RCCL.

Every field (u_n, v_n, u_s, v_s, p) is an n x n grid stored row-major; rank k owns grid rows
[r0, r1) of every field.  A rank's vector is laid out "owned first, then ghosts":

    owned:  field-major, f * L*n + (gr - r0)*n + c                  (L = r1 - r0)
    ghosts: h rows above (r0-h .. r0-1) of every field, then h rows below (r1 .. r1+h-1) of every
            field (periodic): above row j of field f at (f*h + j)*n, below at (nf*h + f*h + j)*n

Matrices keep their global row order inside a rank and have their columns renumbered into that
layout (``DeviceCSR.extract``), so every local row sum is the global one, bit for bit.  Before a
sweep reads a vector its ghost rows are refreshed while the rows that touch no ghost (the interior)
are computed; the boundary rows run after.  Two exchange implementations:

* ``RcclHalo`` (default with the nccl = RCCL backend): libmpbp's own RCCL communicator; the exchange is
  issued from C inside ``mpbp_schur_apply`` (no Python between the kernels): a four-field vector's
  boundary rows are packed by one gather kernel, then one RCCL group of neighbour ncclSend / ncclRecv
  writes straight into the ghost rows, in order on the apply stream (``MPBP_HALO_IN_ORDER``, default; a
  side-stream variant forked / joined by events is ``halo_overlap=True``).  With the communication-
  avoiding schedule (``ca``) an apply makes two such exchanges.
* ``HaloExchanger`` (gloo, CPU-staged; the tests' backend): packs the top/bottom h owned rows of every
  field, all-gathers them, copies the neighbours' strips into the ghost slots.

The halo depth h of each vector kind is measured from the matrices that read it (F, D read
velocity: h = 1; G, Gt_G, Gt_F_G read pressure: h = 2 for Gt_F_G).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_handle
from .csr import DeviceCSR, spgemm
from .mg import FIELDS_PRESSURE, FIELDS_VELOCITY, level_sizes
from .preconditioner import MultiphaseBlockPreconditioner, PGStencil
from .solve import (InnerSolver, PlanProfiling, _capture, _check_f_mode, _check_layout, _check_numerics, _check_pg_mode,
                    _f_stencil, _fill_plan, _pg_stencil)

N_VEL_FIELDS = 4
N_P_FIELDS = 1


@dataclass
class RowPartition:
    n: int
    world: int
    rank: int
    ghosts: bool = False   # ghost slots even at world = 1 (the periodic self-exchange; tests the halo path)
    bounds: tuple | None = None   # explicit ((r0, rows) per rank); default: n split evenly (the first n % world +1)
    allow_empty: bool = False     # coarse multigrid levels (level_partitions) may leave a rank without rows

    def __post_init__(self):
        self.ghosts = self.ghosts or self.world > 1
        if self.bounds is None:
            base, rem = divmod(self.n, self.world)
            self.bounds = tuple((k * base + min(k, rem), base + (1 if k < rem else 0)) for k in range(self.world))
        self.bounds = tuple((int(a), int(b)) for a, b in self.bounds)
        if len(self.bounds) != self.world or sum(b for _, b in self.bounds) != self.n:
            raise ValueError(f"row bounds {self.bounds} do not cover the {self.n} grid rows once")
        start = 0   # contiguous, in rank order, every rank at least one row (the halo and gather layouts assume it)
        for k, (a, b) in enumerate(self.bounds):
            if a != start or b < (0 if self.allow_empty else 1):
                raise ValueError(f"row bounds {self.bounds}: rank {k} must start at row {start} and own "
                                 f"{'>= 0 rows' if self.allow_empty else '>= 1 row'}")
            start += b
        self.r0, self.L = self.bounds[self.rank]
        self.r1 = self.r0 + self.L
        self.min_rows = min(b for _, b in self.bounds)

    def coarse(self, levels: int = 1) -> "RowPartition | None":
        """The same ranks' rows of the grid coarsened `levels` times by 2 (rows [r0 / 2^l, r1 / 2^l)), or None when
        some rank's rows do not halve exactly."""
        f = 1 << levels
        if self.n % f or any(a % f or b % f for a, b in self.bounds):
            return None
        return RowPartition(self.n // f, self.world, self.rank, self.ghosts, tuple((a // f, b // f) for a, b in self.bounds),
                            allow_empty=True)

    @property
    def N(self):
        return self.n * self.n

    def n_owned(self, nfields):
        return nfields * self.L * self.n

    def n_ext(self, nfields, h):
        return self.n_owned(nfields) + (nfields * 2 * h * self.n if self.ghosts else 0)

    def owned_rows(self, nfields) -> np.ndarray:
        """Global ids (in a field-major vector of nfields fields) of the owned unknowns, local order."""
        n, N = self.n, self.N
        return np.concatenate([f * N + np.arange(self.r0 * n, self.r1 * n, dtype=np.int64) for f in range(nfields)])

    def ext_rows(self, nfields, h) -> np.ndarray:
        """Global id of every slot of the owned + ghost ("ext") layout: owned rows field-major, then h rows
        above of every field (increasing row order), then h rows below of every field (periodic)."""
        n, N = self.n, self.N
        cols = np.arange(n, dtype=np.int64)
        above = [f * N + ((self.r0 - h + j) % n) * n + cols for f in range(nfields) for j in range(h)]
        below = [f * N + ((self.r1 + j) % n) * n + cols for f in range(nfields) for j in range(h)]
        parts = [self.owned_rows(nfields)] + (above + below if self.ghosts else [])
        return np.concatenate(parts)

    def colmap(self, nfields, h) -> np.ndarray:
        """Global column -> local ext index (-1 where the rank holds no copy)."""
        n, N, L = self.n, self.N, self.L
        cm = np.full(nfields * N, -1, dtype=np.int32)
        own = self.n_owned(nfields)
        if self.world > 1:
            if self.min_rows < h:
                raise ValueError(f"halo depth {h} exceeds the {self.min_rows} grid rows of the smallest rank")
            cols = np.arange(n, dtype=np.int64)
            for f in range(nfields):
                for j in range(h):
                    top = (self.r0 - h + j) % n
                    bot = (self.r1 + j) % n
                    cm[f * N + top * n + cols] = own + (f * h + j) * n + cols
                    cm[f * N + bot * n + cols] = own + (nfields * h + f * h + j) * n + cols
        for f in range(nfields):
            cm[f * N + self.r0 * n: f * N + self.r1 * n] = f * L * n + np.arange(L * n, dtype=np.int32)
        return cm


def _row_diagonal(M, row_gid: torch.Tensor) -> torch.Tensor:
    """Diagonal of a row subset of an operator with global columns (row i of M is global row row_gid[i])."""
    counts = (M.row_ptr[1:] - M.row_ptr[:-1]).to(torch.int64)
    owner = torch.repeat_interleave(torch.arange(M.shape[0], device=M.col_idx.device), counts)
    hit = M.col_idx.to(torch.int64) == row_gid.to(torch.int64)[owner]
    d = torch.zeros(M.shape[0], dtype=torch.float64, device=M.val.device)
    d[owner[hit]] = M.val[hit]
    if int(hit.sum()) != M.shape[0]:
        raise _lib.MpbpError("rank-local product: a row has no diagonal entry")
    return d


def _gtg_stencil(D, G):
    """The matrix-free Gt_G policy of the global product (commutator_products), for a rank-local product."""
    sd, sg = getattr(D, "stencil", None), getattr(G, "stencil", None)
    if isinstance(sd, PGStencil) and sd.op == _lib.PG_D and isinstance(sg, PGStencil) and sg.op == _lib.PG_G \
            and sd.same_grid(sg):
        return PGStencil(sd.prm, sd.cell, _lib.PG_GTG)
    return None


def halo_reach(row_ptr: torch.Tensor, col_idx: torch.Tensor, row_gid: torch.Tensor, n: int) -> int:
    """Largest periodic grid-row distance between a row and the columns it reads."""
    N = n * n
    counts = (row_ptr[1:] - row_ptr[:-1]).to(torch.int64)
    if col_idx.numel() == 0:
        return 0
    rgr = torch.repeat_interleave((row_gid.to(torch.int64) % N) // n, counts)
    cgr = (col_idx.to(torch.int64) % N) // n
    d = torch.remainder(cgr - rgr, n)
    return int(torch.minimum(d, n - d).max().item())


def ghost_depth(col_idx: torch.Tensor, n: int, r0: int, L: int) -> int:
    """Deepest ghost row the columns `col_idx` (global ids of stacked n x n fields) reach outside the owned grid
    rows [r0, r0 + L), periodic; 0 when every column is owned."""
    if col_idx.numel() == 0:
        return 0
    gr = (col_idx.to(torch.int64) % (n * n)) // n
    above = torch.remainder(r0 - gr, n)          # rows above r0 (1 = the row just above)
    below = torch.remainder(gr - (r0 + L - 1), n)   # rows below the last owned row
    inside = torch.remainder(gr - r0, n) < L
    d = torch.where(inside, torch.zeros_like(gr), torch.minimum(above, below))
    return int(d.max().item())


def boundary_ranges(row_ptr: torch.Tensor, col_idx: torch.Tensor, n_owned_cols: int):
    """(interior, boundary) lists of [a, b) row ranges: a boundary row reads a ghost column."""
    nrows = row_ptr.numel() - 1
    counts = (row_ptr[1:] - row_ptr[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(nrows, device=col_idx.device), counts)
    flag = torch.zeros(nrows, dtype=torch.bool, device=col_idx.device)
    flag[rows[col_idx.to(torch.int64) >= n_owned_cols]] = True
    f = flag.cpu().numpy().astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[-1], f, [-1]])) != 0)
    inner, bnd = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        (bnd if f[a] else inner).append((int(a), int(b)))
    return inner, bnd


class HaloExchanger:
    """All-gather of every rank's top/bottom h owned rows per field; ghosts filled from neighbours."""

    def __init__(self, part: RowPartition, nfields: int, h: int, device, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.part, self.nf, self.h, self.group = part, nfields, h, group
        self.hn = h * part.n
        self.device = torch.device(device)
        backend = dist.get_backend(group)
        self.stage_cpu = backend != "nccl" and self.device.type != "cpu"
        bdev = torch.device("cpu") if self.stage_cpu else self.device
        self.send = torch.empty(nfields * 2 * self.hn, dtype=torch.float64, device=bdev)
        self.recv = torch.empty(part.world * nfields * 2 * self.hn, dtype=torch.float64, device=bdev)
        self.use_base = backend == "nccl"
        self.work = None

    def _pack(self, x_ext):
        own = x_ext[: self.part.n_owned(self.nf)].view(self.nf, self.part.L * self.part.n)
        s = (torch.empty(self.nf, 2, self.hn, dtype=torch.float64, device=x_ext.device)
             if self.stage_cpu else self.send.view(self.nf, 2, self.hn))
        s[:, 0] = own[:, : self.hn]
        s[:, 1] = own[:, own.shape[1] - self.hn:]
        if self.stage_cpu:
            self.send.copy_(s.reshape(-1))

    def begin(self, x_ext: torch.Tensor):
        self._pack(x_ext)
        if self.use_base:
            self.work = self.dist.all_gather_into_tensor(self.recv, self.send, group=self.group, async_op=True)
        else:
            chunks = list(self.recv.view(self.part.world, -1).unbind(0))
            self.work = self.dist.all_gather(chunks, self.send, group=self.group, async_op=True)

    def end(self, x_ext: torch.Tensor):
        if self.work is not None:
            self.work.wait()
            self.work = None
        k, W = self.part.rank, self.part.world
        R = self.recv.view(W, self.nf, 2, self.hn)
        g = x_ext[self.part.n_owned(self.nf): self.part.n_ext(self.nf, self.h)].view(2, self.nf, self.hn)
        g[0] = R[(k - 1) % W, :, 1].to(g.device, non_blocking=True)     # rows above: up's bottom rows
        g[1] = R[(k + 1) % W, :, 0].to(g.device, non_blocking=True)     # rows below: down's top rows

    def exchange(self, x_ext):
        self.begin(x_ext)
        self.end(x_ext)


class Gatherer:
    """All-gather of a row-partitioned nf-field vector into the whole field-major vector (gloo / host-staged; the
    RCCL form is mpbp_halo_allgather): rank k owns rows [r0_k, r0_k + L_k) of every field of an n x n grid."""

    def __init__(self, nf: int, n: int, bounds, rank: int, group=None):
        import torch.distributed as dist
        self.dist, self.group, self.nf, self.n, self.rank = dist, group, nf, n, rank
        self.bounds = tuple(bounds)
        self.lmax = max(b for _, b in self.bounds)
        per = nf * self.lmax * n
        self.send = torch.zeros(per, dtype=torch.float64)
        self.recv = torch.zeros(len(self.bounds) * per, dtype=torch.float64)
        idx = np.empty(nf * n * n, dtype=np.int64)
        for k, (r0, L) in enumerate(self.bounds):
            for f in range(nf):
                idx[f * n * n + r0 * n: f * n * n + (r0 + L) * n] = k * per + f * self.lmax * n + np.arange(L * n)
        self.idx = torch.from_numpy(idx)

    def gather(self, x_owned: torch.Tensor, x_full: torch.Tensor):
        L = self.bounds[self.rank][1]
        own = x_owned[: self.nf * L * self.n].view(self.nf, L * self.n).cpu()
        self.send.view(self.nf, self.lmax * self.n)[:, : L * self.n] = own
        chunks = list(self.recv.view(len(self.bounds), -1).unbind(0))
        self.dist.all_gather(chunks, self.send, group=self.group)
        x_full[: self.idx.numel()] = self.recv[self.idx].to(x_full.device)


def rccl_library_path() -> str:
    """The RCCL torch itself loaded (one RCCL per process), else ROCm's."""
    p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return p if os.path.exists(p) else "/opt/rocm/lib/librccl.so"


class RcclHalo:
    """Ghost-row exchange in libmpbp (csrc/halo.cpp): one gather kernel packs a four-field vector's
    boundary rows (before the group opens), then one RCCL group of neighbour sends / receives writes the
    ghost rows; issued from C inside mpbp_schur_apply -- no Python callback, no all-gather.
    The communicator is libmpbp's own (its unique id travels over `group`); world = 1 exchanges with
    itself (the periodic wrap)."""

    # one RCCL communicator per process group: the first RcclHalo of a group opens it (collective), later ones -- the
    # partitioned preconditioners and their multigrid levels -- share it (mpbp_halo_create_shared, local), so a rank
    # holds one communicator however many preconditioners it builds.  The key is the group's global ranks (stable, unlike
    # id(group)), and whether to share is agreed over the group (an all-reduce MIN of "this rank has a live one"): if
    # any rank lacks it, every rank opens a new communicator together, so no rank waits in a collective the others skip.
    _by_group: dict = {}

    @staticmethod
    def _group_key(part: RowPartition, group):
        import torch.distributed as dist
        g = group if group is not None else dist.group.WORLD
        return (tuple(dist.get_process_group_ranks(g)), part.world, part.rank)

    @staticmethod
    def _agree(have: bool, part: RowPartition, group) -> bool:
        if part.world == 1:
            return have
        import torch.distributed as dist
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.tensor([1 if have else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
        return bool(t.item())

    def __init__(self, part: RowPartition, h_u: int, h_p: int, group=None, overlap: bool = False, share: bool = True):
        """share=False opens a communicator of this object's own (collective over `group`, every rank must pass the same
        value); share=True attaches to the group's existing one when every rank still holds it."""
        import weakref
        key = self._group_key(part, group) if share else None
        ref = RcclHalo._by_group.get(key) if share else None
        base = ref() if ref is not None else None
        have = base is not None and bool(base.handle)
        if share and self._agree(have, part, group):
            self.handle = ctypes.c_void_p()
            check(lib().mpbp_halo_create_shared(base.handle, part.n, part.r0, part.L, h_u, h_p,
                                                ctypes.byref(self.handle)))
            self._finish(overlap)
            return
        path = rccl_library_path().encode()
        uid = (ctypes.c_uint8 * 128)()
        if part.world == 1:
            check(lib().mpbp_rccl_unique_id(path, uid))
        else:
            import torch.distributed as dist
            box = [None]
            if part.rank == 0:
                check(lib().mpbp_rccl_unique_id(path, uid))
                box = [bytes(uid)]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0,
                                       group=group)
            ctypes.memmove(uid, box[0], 128)
        self.handle = ctypes.c_void_p()
        check(lib().mpbp_halo_create(path, uid, part.world, part.rank, part.n, part.r0, part.L, h_u, h_p,
                                     ctypes.byref(self.handle)))
        if share:
            RcclHalo._by_group[key] = weakref.ref(self)
        self._finish(overlap)

    @property
    def comm(self) -> int:
        """Identity of the RCCL communicator this object exchanges over (mpbp_halo_comm)."""
        return int(lib().mpbp_halo_comm(self.handle) or 0)

    @property
    def comm_refs(self) -> int:
        """Halo objects of this process holding the same communicator."""
        return int(lib().mpbp_halo_comm_refs(self.handle))

    def _finish(self, overlap):
        check(lib().mpbp_halo_set_mode(self.handle, _lib.HALO_OVERLAP if overlap else _lib.HALO_IN_ORDER))
        self.overlap = overlap
        self.fn = _lib.HALO_FN(ctypes.cast(lib().mpbp_halo_exchange, ctypes.c_void_p).value)
        self.pair_fn = _lib.HALO_PAIR_FN(ctypes.cast(lib().mpbp_halo_exchange_pair, ctypes.c_void_p).value)
        self.gather_fn = _lib.GATHER_FN(ctypes.cast(lib().mpbp_halo_allgather, ctypes.c_void_p).value)

    def add_kind(self, part: RowPartition, nfields: int, h: int, overlap: bool | None = None) -> int:
        """Another vector layout on this communicator (mpbp_halo_add_kind); returns its kind id."""
        ov = self.overlap if overlap is None else overlap
        return check(lib().mpbp_halo_add_kind(self.handle, nfields, part.n, part.r0, part.L, h,
                                              _lib.HALO_OVERLAP if ov else _lib.HALO_IN_ORDER))

    def add_gather(self, nfields: int, n: int, bounds) -> int:
        """An all-gather layout (mpbp_halo_add_gather): bounds = ((r0, rows) per rank)."""
        r0s = np.ascontiguousarray([a for a, _ in bounds], dtype=np.int32)
        rows = np.ascontiguousarray([b for _, b in bounds], dtype=np.int32)
        return check(lib().mpbp_halo_add_gather(self.handle, nfields, n, r0s.ctypes.data_as(ctypes.c_void_p),
                                                rows.ctypes.data_as(ctypes.c_void_p)))

    def check(self):
        if lib().mpbp_halo_status(self.handle) != 0:
            raise _lib.MpbpError(lib().mpbp_halo_last_error(self.handle).decode())

    def close(self):
        if self.handle:
            lib().mpbp_halo_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Halos:
    """The ghost-row exchanges and all-gathers of one partitioned object: RCCL (libmpbp's halo object; the callbacks
    are its C functions) or torch / gloo (host-staged; Python callbacks looked up by vector address)."""

    def __init__(self, impl: str, rccl: "RcclHalo | None", group, device):
        self.impl, self.rccl, self.group, self.device = impl, rccl, group, torch.device(device)
        self._ex, self._gather, self._tensors = {}, {}, {}
        if rccl is not None:
            self.fn, self.gather_fn, self.ctx = rccl.fn, rccl.gather_fn, rccl.handle
        else:
            self.fn = _lib.HALO_FN(self._halo)
            self.gather_fn = _lib.GATHER_FN(self._allgather)
            self.ctx = None

    def add_kind(self, part: RowPartition, nfields: int, h: int, kind: int | None = None) -> int:
        if self.rccl is not None:
            return self.rccl.add_kind(part, nfields, h) if kind is None else kind
        k = len(self._ex) if kind is None else kind
        while kind is None and k in self._ex:
            k += 1
        self._ex[k] = HaloExchanger(part, nfields, h, self.device, self.group)
        return k

    def add_gather(self, nfields: int, n: int, bounds, rank: int) -> int:
        if self.rccl is not None:
            return self.rccl.add_gather(nfields, n, bounds)
        g = len(self._gather)
        self._gather[g] = Gatherer(nfields, n, bounds, rank, self.group)
        return g

    def register(self, *tensors):
        for t in tensors:
            self._tensors[t.data_ptr()] = t

    # ctypes prints and swallows an exception raised inside a callback, and the C apply would go on with stale ghost
    # rows: the callbacks record the first failure instead, and check() raises it once the apply has returned (as
    # RcclHalo.check does with mpbp_halo_status)
    error = None

    def _halo(self, ctx, kind, x_ptr, phase, stream):
        if self.error is not None:
            return
        try:
            x = self._tensors[int(x_ptr)]
            ex = self._ex[int(kind)]
            if phase == _lib.HALO_BEGIN:
                ex.begin(x)
            else:
                ex.end(x)
        except BaseException as e:   # noqa: BLE001 -- re-raised by check()
            self.error = e

    def _allgather(self, ctx, gid, own_ptr, full_ptr, stream):
        if self.error is not None:
            return
        try:
            self._gather[int(gid)].gather(self._tensors[int(own_ptr)], self._tensors[int(full_ptr)])
        except BaseException as e:   # noqa: BLE001
            self.error = e

    def check(self):
        """Raise the first exception a host-staged exchange or gather hit during the last apply."""
        if self.rccl is not None:
            self.rccl.check()
        if self.error is not None:
            e, self.error = self.error, None
            raise RuntimeError(f"halo exchange failed inside the apply: {type(e).__name__}: {e}") from e


def level_partitions(part: RowPartition, sizes) -> list[RowPartition]:
    """The row partition of every multigrid level: level l + 1's rows of a rank are [ceil(r0 / 2), ceil(r1 / 2)) of its
    level-l rows [r0, r1) -- exact halving for even bounds, a disjoint cover of the coarse grid in any case."""
    parts = [part]
    for m in sizes[1:]:
        p = parts[-1]
        b = tuple(((a + 1) // 2, (a + L + 1) // 2 - (a + 1) // 2) for a, L in p.bounds)
        parts.append(RowPartition(m, part.world, part.rank, part.ghosts, b, allow_empty=True))
    return parts


def _csr_rows(M: DeviceCSR, idx: torch.Tensor) -> DeviceCSR:
    """Rows idx (local row numbers of M, device) of M in that order: entries and their order kept, columns as they are."""
    rp = M.row_ptr.to(torch.int64)
    idx = idx.to(torch.int64)
    lens = rp[idx + 1] - rp[idx]
    nrp = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=rp.device)
    torch.cumsum(lens, 0, out=nrp[1:])
    owner = torch.repeat_interleave(torch.arange(idx.numel(), device=rp.device), lens)
    src = rp[idx][owner] + (torch.arange(int(nrp[-1]), device=rp.device) - nrp[:-1][owner])
    return DeviceCSR(nrp.to(torch.int32), M.col_idx[src].contiguous(), M.val[src].contiguous(), (idx.numel(), M.shape[1]))


def _positions(keys: torch.Tensor, v: torch.Tensor, bad: torch.Tensor | None = None) -> torch.Tensor:
    """Positions of the values v in the sorted `keys` (every value must be a key).  bad (a device bool, optional):
    OR-ed with "some value is not a key" and left for the caller to check once (no device synchronisation here);
    without it the check is made at once."""
    k = keys.to(torch.int64)
    vv = v.to(torch.int64)
    pos = torch.searchsorted(k, vv)
    if v.numel():
        miss = (pos >= k.numel()) | (k[pos.clamp(max=max(k.numel() - 1, 0))] != vv)
        if bad is not None:
            bad |= miss.any()
        elif bool(miss.any()):
            raise ValueError("a row / column outside this rank's band")
    return pos


def _relabel_cols(M: DeviceCSR, keys: torch.Tensor, bad: torch.Tensor | None = None) -> DeviceCSR:
    """M with every column replaced by its position in the sorted `keys`: the same entries in the same order (the
    relabelling is monotone), as a product's left operand indexing the rows `keys` of the right one."""
    return DeviceCSR(M.row_ptr, _positions(keys, M.col_idx, bad).to(torch.int32), M.val, (M.shape[0], keys.numel()))


def _allgather_csr(M: DeviceCSR, rows: torch.Tensor, nrows: int, group) -> DeviceCSR:
    """The whole operator from every rank's rows: M holds the global rows `rows` of this rank (global columns); the
    result has every one of the `nrows` rows in global order, each row's entries in their order."""
    import torch.distributed as dist
    dev = M.val.device
    cdev = dev if dist.get_backend(group) == "nccl" else torch.device("cpu")
    world = dist.get_world_size(group)
    lens = (M.row_ptr[1:] - M.row_ptr[:-1]).to(torch.int64)
    meta = torch.tensor([rows.numel(), M.col_idx.numel()], dtype=torch.int64, device=cdev)
    metas = [torch.empty_like(meta) for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    cnt = [(int(m[0]), int(m[1])) for m in metas]

    def gather(t, k, dtype):
        size = max(max(c[k] for c in cnt), 1)
        buf = torch.zeros(size, dtype=dtype, device=cdev)
        buf[: t.numel()] = t.to(device=cdev, dtype=dtype)
        outs = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(outs, buf, group=group)
        return torch.cat([o[: c[k]] for o, c in zip(outs, cnt)]).to(dev)
    r_all, l_all = gather(rows, 0, torch.int64), gather(lens, 0, torch.int64)
    c_all, v_all = gather(M.col_idx, 1, torch.int64), gather(M.val, 1, torch.float64)
    perm = torch.argsort(r_all)
    if r_all.numel() != nrows or not bool((r_all[perm] == torch.arange(nrows, device=dev)).all()):
        raise ValueError("the ranks' rows do not cover the level exactly once")
    start = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(l_all, 0, out=start[1:])
    ls = l_all[perm]
    rp = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(ls, 0, out=rp[1:])
    owner = torch.repeat_interleave(torch.arange(nrows, device=dev), ls)
    src = start[perm][owner] + (torch.arange(int(rp[-1]), device=dev) - rp[:-1][owner])
    return DeviceCSR(rp.to(torch.int32), c_all[src].to(torch.int32).contiguous(), v_all[src].contiguous(),
                     (nrows, M.shape[1]))


def mg_part_cap(sizes, part: RowPartition, nfields: int, min_cells: int = 1 << 14,
                max_part_levels: int | None = None) -> int:
    """The levels [0, cap) a row-partitioned hierarchy may split by size alone: PartitionedMultigrid's rule without
    the ghost-depth test (which can only stop it earlier)."""
    nl = len(sizes)
    parts = level_partitions(part, sizes)
    cap = nl - 1 if max_part_levels is None else max(1, min(nl - 1, max_part_levels))
    for l in range(1, nl - 1):
        q = parts[l]
        if l >= cap or nfields * q.n * q.n // part.world < min_cells or q.min_rows < 1:
            return l
    return nl - 1


def mg_bands(sizes, fields, part: RowPartition, cap: int, device) -> list:
    """S_l, l = 0 .. cap: the rows of level l (sorted global ids, device int32) a rank forms to have its owned rows of
    every level down to `cap`: S_cap = the owned rows, S_l = the owned rows and every fine row the restriction of
    S_{l+1} reads (A_{l+1} = R_l (A_l P_l) row by row needs exactly those rows of A_l)."""
    from .mg import transfer_rows
    nf = len(fields)
    parts = level_partitions(part, sizes)
    own = [torch.from_numpy(q.owned_rows(nf).astype(np.int32)).to(device) for q in parts[: cap + 1]]
    S = [None] * (cap + 1)
    S[cap] = own[cap]
    for l in range(cap - 1, -1, -1):
        R = transfer_rows(sizes[l], fields, _lib.MG_R, S[l + 1])
        S[l] = torch.unique(torch.cat([own[l], R.col_idx])).to(torch.int32)
    return S


class LocalHierarchy:
    """The multigrid levels one rank of a row partition needs, formed from its own rows: no global operator on any
    rank (setup memory O(N / world + ghosts) down to the replicated coarse levels).

    A0 holds the rows S[0] (mg_bands) of level 0's operator with their global columns (assembled, or the rank-local
    product rows of Gt_G).  Level l + 1's band is R_l[S_{l+1}] (A_l[S_l] P_l) with the restriction's columns relabelled
    into S_l and A_l's into the fine rows it reaches (monotone relabellings: each product row performs the global
    SpGEMM's operations in its order -- the one-GPU hierarchy's rows bit for bit), the transfers' rows built for those
    rows only (mpbp_mg_transfer_rows_*).  replicated(P) all-gathers the ranks' owned rows of level P and coarsens
    that level as mg.Multigrid does (the levels below are small): the same operators as the one-GPU hierarchy's."""

    def __init__(self, A0: DeviceCSR, S: list, sizes, fields, part: RowPartition, group=None, pre=2, post=2,
                 cycles=1, ratio=4.0, coarsest=8, stamp=None):
        from .mg import transfer_rows
        stamp = stamp or (lambda name: None)
        self.device = A0.val.device
        self.sizes, self.fields, self.n, self.nf = list(sizes), tuple(fields), int(sizes[0]), len(fields)
        self.nlevels = len(self.sizes)
        self.pre, self.post, self.cycles, self.ratio, self.coarsest = pre, post, cycles, ratio, coarsest
        self.S, self.part, self.group = S, part, group
        if A0.shape[0] != S[0].numel():
            raise ValueError("A0 must hold the band rows S[0]")
        self.band = [A0]
        bad = torch.zeros((), dtype=torch.bool, device=self.device)   # checked once (each sync costs under contention)
        for l in range(len(S) - 1):
            A = self.band[l]
            C = torch.unique(A.col_idx)
            AP = spgemm(_relabel_cols(A, C, bad), transfer_rows(self.sizes[l], self.fields, _lib.MG_P, C))
            R = transfer_rows(self.sizes[l], self.fields, _lib.MG_R, S[l + 1])
            self.band.append(spgemm(_relabel_cols(R, S[l], bad), AP))
            del AP, R
            stamp(f"mg_band_level{l + 1}")
        if bool(bad):
            raise ValueError("LocalHierarchy: a restriction row reads outside its band (mg_bands)")
        self._rep = {}
        self.stamp = stamp

    def op_rows(self, l: int, rows: torch.Tensor) -> DeviceCSR:
        return _csr_rows(self.band[l], _positions(self.S[l], rows))

    def R_rows(self, l: int, rows: torch.Tensor) -> DeviceCSR:
        from .mg import transfer_rows
        return transfer_rows(self.sizes[l], self.fields, _lib.MG_R, rows)

    def P_rows(self, l: int, rows: torch.Tensor) -> DeviceCSR:
        from .mg import transfer_rows
        return transfer_rows(self.sizes[l], self.fields, _lib.MG_P, rows)

    def diag_rows(self, l: int, rows: torch.Tensor) -> torch.Tensor:
        return _row_diagonal(self.op_rows(l, rows), rows)

    def bounds(self, l: int, rows: torch.Tensor):
        """(lmin, lmax) of level l's smoother: the Gershgorin bound is the maximum over the ranks of their owned rows'
        (every row's sum is the global operator's): the one-GPU hierarchy's bound, exactly."""
        import torch.distributed as dist
        lm = self.op_rows(l, rows).gershgorin(self.diag_rows(l, rows)) if rows.numel() else 0.0
        cdev = self.device if dist.get_backend(self.group) == "nccl" else "cpu"
        t = torch.tensor([lm], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        lmax = float(t.item())
        return lmax / self.ratio, lmax

    def replicated(self, P: int):
        """mg.Multigrid of level P's whole operator (every rank's owned rows of it, all-gathered): levels P .. end."""
        if P not in self._rep:
            from .mg import Multigrid
            q = level_partitions(self.part, self.sizes)[P]
            own = torch.from_numpy(q.owned_rows(self.nf).astype(np.int32)).to(self.device)
            full = _allgather_csr(self.op_rows(P, own), own, self.nf * self.sizes[P] ** 2, self.group)
            self.stamp("mg_gather_level")
            if P == self.nlevels - 1:   # only the coarsest level: its dense inverse
                self._rep[P] = _CoarsestLevel(full, self.ratio)
            else:
                sub = Multigrid(full, self.sizes[P], self.fields, pre=self.pre, post=self.post, cycles=self.cycles,
                                ratio=self.ratio, coarsest=self.coarsest, fine_sell=True)
                if sub.sizes != self.sizes[P:]:
                    raise AssertionError(f"coarse levels {sub.sizes} != {self.sizes[P:]}")
                self._rep[P] = sub
            self.stamp("mg_replicated_levels")
        return self._rep[P]


class _CoarsestLevel:
    """The coarsest level alone (a hierarchy partitioned down to it): its operator, buffers and dense pseudo-inverse, as
    mg.Multigrid holds its last level (the same struct fields, the same inverse)."""

    def __init__(self, A: DeviceCSR, ratio: float):
        from .mg import dense_inverse_csr
        dev = A.val.device
        d = A.diagonal()
        lmax = A.gershgorin(d)
        self.bounds = [(lmax / ratio, lmax)]
        self.A, self.diag = A, d
        self.coarse_inv, inv = dense_inverse_csr(A)
        self.coarse_dense = torch.from_numpy(np.ascontiguousarray(inv.T)).to(dev)
        self.work = [[torch.zeros(A.shape[0], dtype=torch.float64, device=dev) for _ in range(5)]]
        self._levels = (_lib.MgLevel * 1)()
        L = self._levels[0]
        L.nrows = A.shape[0]
        L.lmin, L.lmax = self.bounds[0]
        L.A, L.A_blocks, L.diag = A.cstruct(), A.blocks.cstruct(), d.data_ptr()
        L.R = L.P = _lib.Csr(0, 0, 0, None, None, None)
        L.R_blocks = L.P_blocks = _lib.RowBlocks(None, 0)
        L.x, L.t, L.r, L.d, L.b = (w.data_ptr() for w in self.work[0])


class _GlobalLevels:
    """LocalHierarchy's interface over a whole mg.Multigrid (every rank holds the global hierarchy)."""

    def __init__(self, g):
        self.g = g
        self.device, self.sizes, self.fields, self.n = g.device, g.sizes, g.fields, g.n
        self.nlevels, self.pre, self.post, self.cycles = g.nlevels, g.pre, g.post, g.cycles

    def _rows(self, M, rows):
        return M.extract(rows, torch.arange(M.shape[1], dtype=torch.int32, device=self.device), M.shape[1])

    def op_rows(self, l, rows):
        return self._rows(self.g.ops[l], rows)

    def R_rows(self, l, rows):
        return self._rows(self.g.R[l], rows)

    def P_rows(self, l, rows):
        return self._rows(self.g.P[l], rows)

    def diag_rows(self, l, rows):
        return self.g.diags[l][rows.long()].contiguous()

    def bounds(self, l, rows):
        return self.g.bounds[l]

    def replicated(self, P):
        return _Shifted(self.g, P)


class _Shifted:
    """Levels P .. end of a whole hierarchy, numbered from 0 (LocalHierarchy.replicated's form)."""

    def __init__(self, g, P):
        self.g, self.P = g, P
        self._levels = g._levels[P:]
        self.work = g.work[P:]
        self.bounds = g.bounds[P:]
        self.coarse_inv, self.coarse_dense = g.coarse_inv, g.coarse_dense


class PartitionedMultigrid:
    """A multigrid hierarchy (mg.Multigrid, built on every rank from the global operator -- setup only) split over a
    row partition for the partitioned Schur apply (solve.py:266 / 274's pointer, under north_star's row partition).

    Level l + 1's rows of rank k are [ceil(r0 / 2), ceil(r1 / 2)) of its level-l rows [r0, r1) (exact halving when
    the rows are even; a disjoint cover of the coarse grid in any case).  Levels [0, part_levels) are row-partitioned:
    their operator, restriction and prolongation rows extracted with the columns renumbered into the ghost layout
    (entry order kept), their vectors owned + ghost rows, ghost depths measured from the columns.  The restriction
    into level part_levels leaves each rank's rows of that level, all-gathered into the whole level; the coarser
    levels (and the dense coarsest inverse) run replicated on every rank.  Every operation is the one-GPU hierarchy's
    on the same operands: bit-identical to Multigrid.solve / the one-GPU apply.  Partitioning stops at the coarsest
    level, where a rank would hold fewer rows than the ghost depth, or below min_cells unknowns per rank."""

    def __init__(self, g, part: RowPartition, nfields: int, group=None, min_cells: int = 1 << 14,
                 max_part_levels: int | None = None):
        # g: a LocalHierarchy (this rank's rows only) or a whole mg.Multigrid (every rank holds it)
        if getattr(g, "coarsen", "even") != "even":
            raise ValueError(f"coarsen={g.coarsen!r} is not available under the row partition: the rows' halving and "
                             'ghost depths assume 2:1 transfers; use coarsen="even" here')
        if getattr(g, "smoother", "point") != "point":
            raise ValueError(f"smoother={g.smoother!r} is one GPU only: the row partition runs the point smoother "
                             '(use smoother="point" here)')
        g = g if isinstance(g, LocalHierarchy) else _GlobalLevels(g)
        self.g, self.part0, self.nf, self.group = g, part, nfields, group
        dev = g.device
        self.device = dev
        nl = g.nlevels
        self.parts = level_partitions(part, g.sizes)
        world = part.world

        def owned(l):
            return torch.from_numpy(self.parts[l].owned_rows(nfields).astype(np.int32)).to(dev)

        def depth(full, l):   # ghost rows of level l read by the rows `full` (global columns at level l)
            if world == 1:
                return 1
            q = self.parts[l]
            return ghost_depth(full.col_idx, q.n, q.r0, q.L)

        def reduce_max(v):
            if world == 1:
                return v
            import torch.distributed as dist
            t = torch.tensor([v], dtype=torch.int64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            return int(t.item())

        self.h0 = reduce_max(max(1, depth(g.R_rows(0, owned(1)), 0)))   # level 0 ghosts the restriction reads
        self.h = [self.h0]
        P = nl - 1
        cap = nl - 1 if max_part_levels is None else max(1, min(nl - 1, max_part_levels))
        for l in range(1, nl - 1):
            q = self.parts[l]
            cells = nfields * q.n * q.n // world
            hl = reduce_max(max(1, depth(g.op_rows(l, owned(l)), l), depth(g.R_rows(l, owned(l + 1)), l),
                                depth(g.P_rows(l - 1, owned(l - 1)), l)))
            if l >= cap or cells < min_cells or q.min_rows < hl:
                P = l
                break
            self.h.append(hl)
        self.part_levels = P
        self._owned = owned

    def build(self, halos: _Halos, level0, diag0, h0: int, kind0: int | None = None, A0=None, cycles=None):
        """Local operators, vectors and the mpbp_mg struct.  level0: (x, t) iterate buffers of level 0 (owned + ghost
        rows at depth h0 >= self.h0; inside the Schur apply its own); diag0: level 0's owned diagonal; kind0: level 0's
        halo kind (the Schur apply's velocity / pressure kind; None: a new one); A0: level 0's local operator for the
        standalone solve (mpbp_mg_solve; None inside the Schur apply, whose level 0 is its own operator)."""
        g, nf, P, dev = self.g, self.nf, self.part_levels, self.device
        rep = g.replicated(P)   # levels P .. end, whole on every rank
        if h0 < self.h0:
            raise ValueError(f"level 0 ghost depth {h0} < the restriction's {self.h0}")
        self.h[0] = h0
        from .mg import sell_copy
        f64 = dict(dtype=torch.float64, device=dev)
        self.kinds, self.local, self.work = [], [], []
        for l in range(P):
            q = self.parts[l]
            self.kinds.append(halos.add_kind(q, nf, self.h[l]) if (l > 0 or kind0 is None) else kind0)
        gather_bounds = self.parts[P].bounds
        self.gather_kind = halos.add_gather(nf, self.parts[P].n, gather_bounds, self.part0.rank)
        self._levels = (_lib.MgLevel * g.nlevels)()
        empty_sell = _lib.Sell(0, 0, 0, 0, None, None, None, None)
        keep = []
        for l in range(g.nlevels):
            L = self._levels[l]
            L.pre, L.post = g.pre, g.post
            if l >= P:   # replicated: the whole level
                G = rep._levels[l - P]
                for name, _ in _lib.MgLevel._fields_:
                    setattr(L, name, getattr(G, name))
                L.lmin, L.lmax = rep.bounds[l - P]
                continue
            q = self.parts[l]
            rows = self._owned(l)
            L.lmin, L.lmax = g.bounds(l, rows)
            ext = q.n_ext(nf, self.h[l])
            cm = torch.from_numpy(q.colmap(nf, self.h[l])).to(dev)
            if l + 1 < P:
                qn = self.parts[l + 1]
                cm_next = torch.from_numpy(qn.colmap(nf, self.h[l + 1])).to(dev)
                ext_next = qn.n_ext(nf, self.h[l + 1])
            else:
                ncoarse = nf * g.sizes[l + 1] ** 2
                cm_next, ext_next = torch.arange(ncoarse, dtype=torch.int32, device=dev), ncoarse

            def local(M, cmap, ncols):   # all rows of M (global columns) with the columns into the ghost layout
                return M.extract(torch.arange(M.shape[0], dtype=torch.int32, device=dev), cmap, ncols)
            R = local(g.R_rows(l, self._owned(l + 1)), cm, ext)
            Pm = local(g.P_rows(l, rows), cm_next, ext_next)
            own = q.n_owned(nf)
            L.nrows = own
            if l == 0:
                L.A = A0.cstruct() if A0 is not None else _lib.Csr(0, 0, 0, None, None, None)
                L.A_blocks = A0.blocks.cstruct() if A0 is not None else _lib.RowBlocks(None, 0)
                L.diag = diag0.data_ptr()
                SA = sell_copy(A0) if A0 is not None else None
                L.A_sell = SA.cstruct() if SA is not None else empty_sell
                keep += [A0, SA, diag0]
                x, t = level0
                r = torch.zeros(ext, **f64)
                d, bb = torch.zeros(own, **f64), torch.zeros(own, **f64)
            else:
                A = local(g.op_rows(l, rows), cm, ext)
                dg = g.diag_rows(l, rows)
                L.A, L.A_blocks, L.diag = A.cstruct(), A.blocks.cstruct(), dg.data_ptr()
                SA = sell_copy(A)
                L.A_sell = SA.cstruct() if SA is not None else empty_sell
                keep += [A, dg, SA]
                x, t, r = (torch.zeros(ext, **f64) for _ in range(3))
                d, bb = torch.zeros(own, **f64), torch.zeros(own, **f64)
            SR, SP = sell_copy(R), sell_copy(Pm)
            L.R, L.R_blocks, L.P, L.P_blocks = R.cstruct(), R.blocks.cstruct(), Pm.cstruct(), Pm.blocks.cstruct()
            L.R_sell = SR.cstruct() if SR is not None else empty_sell
            L.P_sell = SP.cstruct() if SP is not None else empty_sell
            keep += [R, Pm, SR, SP]
            L.x, L.t, L.r, L.d, L.b = (v.data_ptr() for v in (x, t, r, d, bb))
            L.halo_kind = self.kinds[l]
            L.part_r0, L.part_h = q.r0, self.h[l]   # (the matrix-free level 1's owned window, k_gal1 / k_gal1p)
            self.work.append((x, t, r, d, bb))
            halos.register(x, t, r, d, bb)
        # the gather level's r (the rank's rows, written by the restriction) and b (the whole level) are the global
        # level's full-size buffers
        Gw = rep.work[0]
        halos.register(*Gw)
        self._keep = keep + [rep]
        self._halos = halos
        self._mg = _lib.Mg(g.nlevels, g.cycles if cycles is None else cycles,
                           ctypes.cast(self._levels, ctypes.POINTER(_lib.MgLevel)),
                           rep.coarse_inv.cstruct(), rep.coarse_inv.blocks.cstruct(),
                           rep.coarse_dense.data_ptr() if rep.coarse_dense is not None else None,
                           P, self.gather_kind, halos.fn, halos.ctx, halos.gather_fn)
        from .mg import set_transfer_kinds
        set_transfer_kinds(self._mg, g.fields, g.n)   # (matrix-free transfers on the replicated levels only)
        return self

    def cstruct(self):
        return self._mg


def _dist_info(group):
    import torch.distributed as dist
    return dist, dist.get_world_size(group), dist.get_rank(group), dist.get_backend(group)


def _phase_clock(out: dict):
    """stamp(name): with MPBP_SETUP_TIMING=1, synchronise the device and record the seconds since the previous stamp
    under `name` in `out`; otherwise nothing (no extra synchronisation in production setups)."""
    if os.environ.get("MPBP_SETUP_TIMING", "0") != "1":
        return lambda name: None
    import time
    torch.cuda.synchronize()
    last = [time.perf_counter()]

    def stamp(name):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out[name] = out.get(name, 0.0) + (t - last[0])
        last[0] = t
    return stamp


def _check_halo(halo: str) -> str:
    if halo not in ("auto", "rccl", "torch"):
        raise ValueError("halo must be 'auto', 'rccl' or 'torch'")
    return halo


class _PartitionedOperator:
    """What the row-partitioned operators of the system share: the partition, the owned + ghost ("ext") input buffer
    ``xe`` with its ghost-row exchange, and the schedule of apply(x) on the rank's owned entries -- x copied into xe,
    the exchange begun, the rows that read no ghost launched, the exchange ended, the boundary rows launched.  The
    exchange is RCCL neighbour point-to-point over xGMI on a communicator of this object's own (its eager exchanges --
    overlap=True: on the halo object's high-priority side stream, forked before and joined after the interior launch
    -- are never mixed with a preconditioner's in-order ones inside a replayed graph on one communicator), or with the
    gloo backend the host-staged HaloExchanger.  A subclass supplies _whole (the unpartitioned apply), _interior and
    _boundary."""

    def __init__(self, n: int, nfields: int, group, halo: str, self_halo: bool):
        _check_halo(halo)
        _, world, rank, backend = _dist_info(group)
        self.nfields = nfields
        self.part = RowPartition(n, world, rank, ghosts=bool(self_halo))
        self.partitioned = self.part.ghosts
        self.halo_impl = halo if halo != "auto" else ("rccl" if backend == "nccl" else "torch")
        self._rccl = self._ex = self.xe = None

    def _open_halo(self, h: int, device, group, overlap: bool):
        """The sizes at ghost depth h and, under a partition, xe and its exchange."""
        part, nf = self.part, self.nfields
        self.h = h
        self.n_own, self.n_ext = part.n_owned(nf), part.n_ext(nf, h)
        self.shape = (self.n_own, self.n_own)
        if not self.partitioned:
            return
        self.xe = torch.zeros(self.n_ext, dtype=torch.float64, device=device)
        if self.halo_impl == "rccl":
            self._rccl = RcclHalo(part, 1, 1, group, overlap=False, share=False)
            self.kind = self._rccl.add_kind(part, nf, h, overlap=overlap)
        else:
            self._ex = HaloExchanger(part, nf, h, device, group)

    def _exchange(self, phase):
        if self._rccl is not None:
            lib().mpbp_halo_exchange(self._rccl.handle, self.kind, ptr(self.xe), phase, stream_handle())
        elif phase == _lib.HALO_BEGIN:
            self._ex.begin(self.xe)
        else:
            self._ex.end(self.xe)

    def apply(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        assert x.is_cuda and x.dtype == torch.float64 and x.numel() == self.n_own
        if out is None:
            out = torch.empty(self.n_own, dtype=torch.float64, device=x.device)
        if not self.partitioned:
            return self._whole(x, out)
        assert out.is_cuda and out.dtype == torch.float64 and out.numel() == self.n_own
        self.xe[: self.n_own].copy_(x)
        self._exchange(_lib.HALO_BEGIN)
        self._interior(out)
        self._exchange(_lib.HALO_END)
        self._boundary(out)
        if self._rccl is not None:
            self._rccl.check()
        return out

    matvec = apply

    def close(self):
        if self._rccl is not None:
            self._rccl.close()
            self._rccl = None

    def local_to_global_rows(self):
        return self.part.owned_rows(self.nfields)


class DistributedMatrix(_PartitionedOperator):
    """A row-partitioned operator of the MAC-grid system: the operator matvec b = A u of apply.py:72 and the FGMRES
    operator of solve.py:285 (A @ xk, solve.py:166) over the ranks of `group`, one per GPU.

    Rank k holds the rows of grid rows [r0, r1) of every one of `nfields` stacked n x n fields (A: the 5 fields
    [u_n, v_n, u_s, v_s, p]), columns renumbered into the owned + ghost ("ext") layout (DeviceCSR.extract keeps each
    row's entry order: every local row sum is the global one, bit for bit).  apply(x) takes and returns the rank's
    owned entries (_PartitionedOperator's schedule): the interior rows (no ghost column) run on the CSR kernel while
    the ghost rows are exchanged, the boundary rows after."""

    def __init__(self, M: DeviceCSR, n: int, nfields: int, group=None, halo: str = "auto", overlap: bool = True,
                 self_halo: bool = False, owned_rows: bool = False):
        """M: the global operator, or (owned_rows=True) just this rank's rows of it, in owned order, with global
        columns (MultiphaseBlockPreconditioner.assemble_rows: rank-local setup)."""
        super().__init__(n, nfields, group, halo, self_halo)
        part, dev = self.part, M.device
        N_all = nfields * n * n
        if M.shape != ((part.n_owned(nfields) if owned_rows else N_all), N_all):
            raise ValueError(f"operator {M.shape} is not {'this rank' + chr(39) + 's rows of ' if owned_rows else ''}"
                             f"{nfields} fields of a {n} x {n} grid")
        rows = torch.from_numpy(part.owned_rows(nfields).astype(np.int32)).to(dev)
        if owned_rows:
            full, rows = M, torch.arange(M.shape[0], dtype=torch.int32, device=dev)
        else:
            full = M.extract(rows, torch.arange(M.shape[1], dtype=torch.int32, device=dev), M.shape[1])
        h = max(1, ghost_depth(full.col_idx, n, part.r0, part.L) if part.world > 1 else 1)
        del full
        if owned_rows and not self.partitioned:
            raise ValueError("owned_rows=True needs a row partition")
        self._open_halo(h, dev, group, overlap)
        self.A = M.extract(rows, torch.from_numpy(part.colmap(nfields, h)).to(dev), self.n_ext) \
            if self.partitioned else M
        # (one rank exchanging with itself: every row with a wrapped neighbour reads ghosts)
        inner, bnd = boundary_ranges(self.A.row_ptr, self.A.col_idx, self.n_own) if self.partitioned else \
            ([(0, self.n_own)], [])
        self.blk_in = self.A.plan_blocks(rows=inner) if inner else None
        self.blk_bd = self.A.plan_blocks(rows=bnd) if bnd else None

    @property
    def device(self):
        return self.A.device

    def _whole(self, x, out):
        return self.A.matvec(x, out=out)

    def _interior(self, out):
        if self.blk_in is not None:
            self.A.matvec(self.xe, out=out, blocks=self.blk_in)

    def _boundary(self, out):
        if self.blk_bd is not None:
            self.A.matvec(self.xe, out=out, blocks=self.blk_bd)


class DistributedStokesOperator(_PartitionedOperator):
    """The row-partitioned system matrix applied matrix-free: DistributedMatrix's surface and schedule with every owned
    row of ``A x`` recomputed from the thn tables (mpbp_stokes_apply_part) -- no row of A assembled, extracted,
    renumbered or planned on any rank.

    op: a StokesOperator (``bp.stokes_operator(c, d_u)``), held by reference: ``bp.update_theta_tables(...)`` and
    ``op.set_params(...)`` are seen by the next apply with no rebuild (there is nothing to refill).  Numerics are
    ``op.numerics``: "exact" gives the rows of the assembled A's product (DistributedMatrix.apply, and the one-GPU
    StokesOperator) bit for bit, "fast" the one-GPU fast operator's rows bit for bit.

    apply(x) takes and returns the rank's owned entries (5 fields, owned grid rows [r0, r1), field-major): x is copied
    into the 5-field ext buffer, the ghost rows (h = 1) are exchanged -- RCCL on a communicator of this object's own
    (overlap=True: on the halo's side stream, across the interior rows' launch) or the host-staged HaloExchanger
    (gloo) -- while the rows 1 .. L-2 (no ghost read) run, and the first and last owned grid rows run after the
    exchange.  Unpartitioned (world 1 without self_halo) apply is ``op.matvec``.

    Needs n >= 3.  Every rank holds the three GLOBAL thn tables (3 n^2 doubles: 100 MB at 2048^2) -- the tables are
    not partitioned."""

    def __init__(self, op, group=None, halo: str = "auto", overlap: bool = True, self_halo: bool = False):
        from .preconditioner import StokesOperator
        if not isinstance(op, StokesOperator):
            raise TypeError("DistributedStokesOperator needs a StokesOperator (MultiphaseBlockPreconditioner.stokes_operator)")
        n = int(op.prm.n)
        if n < 3:
            raise ValueError("DistributedStokesOperator needs n >= 3")
        super().__init__(n, 5, group, halo, self_halo)
        self.op = op
        self._open_halo(1, op.device, group, overlap)
        if self.partitioned:
            self._parts = tuple(_lib.RowPart(self.part.r0, self.part.L, self.h, which, 0, 0) for which in (0, 1, 2))

    @property
    def device(self):
        return self.op.device

    @property
    def numerics(self):
        return self.op.numerics

    def _launch(self, which: int, out, mode=_lib.SPMV_STORE, z=None):
        op = self.op
        flags = int(mode) | (_lib.SPMV_FAST if op.numerics == "fast" else 0)
        check(lib().mpbp_stokes_apply_part(ctypes.byref(op.prm), ptr(op.cell), ptr(op.uface), ptr(op.vface),
                                           ctypes.byref(self._parts[which]), flags, ptr(self.xe), ptr(z), ptr(out),
                                           stream_handle()))

    def _whole(self, x, out):
        return self.op.matvec(x, out=out)

    def _interior(self, out):
        self._launch(1, out)          # rows 1 .. L-2: no ghost row read (nothing launched when L <= 2)

    def _boundary(self, out):
        self._launch(2, out)          # the first and last owned grid rows

    def __repr__(self):
        return (f"DistributedStokesOperator(n={self.part.n}, rows=[{self.part.r0}, {self.part.r1}), "
                f"numerics={self.numerics!r}, halo={self.halo_impl if self.partitioned else None!r})")


def _csr_vstack(A: DeviceCSR, B: DeviceCSR) -> DeviceCSR:
    """The rows of A, then the rows of B (same column count), as one CSR."""
    rp = torch.cat([A.row_ptr[:-1], B.row_ptr + A.nnz])
    return DeviceCSR(rp.contiguous(), torch.cat([A.col_idx, B.col_idx]), torch.cat([A.val, B.val]),
                     (A.shape[0] + B.shape[0], A.shape[1]))


def _q13_block(Q: DeviceCSR, n: int, part, group, red_dev):
    """(n, vals, symmetric) for a row partition: Gt_F_G's diamond over grid rows r0 - 2 .. r0 + L - 1 (Q: those rows
    with global columns, mpbp_q13_build_rows) and whether the product is symmetric to 1e-14 of its largest entry over
    every rank's owned rows (slot s at a cell against slot 12 - s at its neighbour (dr_s, dc_s) -- mpbp_q13_asymmetry's
    test, reduced over the ranks).  None when Q's rows are not the 13-point diamond."""
    import torch.distributed as dist
    L = part.L
    vals = torch.empty(13 * (L + 2) * n, dtype=torch.float64, device=Q.device)
    if lib().mpbp_q13_build_rows(ctypes.byref(Q.cstruct()), n, part.r0 - 2, ptr(vals), stream_handle()) != 0:
        ok = torch.tensor([0.0], dtype=torch.float64, device=red_dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MAX, group=group)   # (the same collective on every rank)
        dist.all_reduce(ok, op=dist.ReduceOp.MAX, group=group)
        return None
    V = vals.view(13, L + 2, n)
    amax = V[:, 2:, :].abs().max()
    asym = torch.zeros((), dtype=torch.float64, device=Q.device)
    dr = (-2, -1, -1, -1, 0, 0)
    dc = (0, -1, 0, 1, -2, -1)
    for s in range(6):
        nb = torch.roll(V[12 - s, 2 + dr[s]: 2 + dr[s] + L, :], shifts=-dc[s], dims=1)
        asym = torch.maximum(asym, (V[s, 2:, :] - nb).abs().max())
    a = torch.stack([asym, amax]).to(red_dev)
    dist.all_reduce(a[0:1], op=dist.ReduceOp.MAX, group=group)
    dist.all_reduce(a[1:2], op=dist.ReduceOp.MAX, group=group)
    a = a.cpu()
    return n, vals, bool(a[0] <= 1e-14 * a[1])


# the apply's five operators: plan key -> (attribute, row kind, column kind); "u": the four velocity fields, "p": pressure
_OPS = {"F": ("F", "u", "u"), "D": ("D", "p", "u"), "G": ("G", "u", "p"), "P": ("GtG", "p", "p"), "Q": ("GtFG", "p", "p")}


class _RowSource:
    """Where a rank's rows of level 0 come from during the partitioned setup.  Two sources, one surface (as
    LocalHierarchy / _GlobalLevels one level down); DistributedSchurPreconditioner picks one and is written once
    against it:

        op[key]                      F / D / G / P (Gt_G) / Q (Gt_F_G), global columns, stencils attached
        q13_rows()                   fast numerics: Gt_F_G's grid rows r0 - 2 .. r0 + L - 1 for _q13_block, else None
        resolve(ik, key)             the inner solver with its Chebyshev interval from the GLOBAL operator's bound
        reach(key)                   the halo reach of the operator on the owned rows
        hierarchy(ik, key, fields)   what PartitionedMultigrid splits: the multigrid levels for one inner solver
        ext_diagonal(key, rows)      the operator's diagonal on owned + ghost rows (the CA schedule)
        owned_ext(key, cmap, ncols)  the owned rows with their columns in the ext layout

    A source holds every setup-only operator and assembly object; dropping it frees them."""

    def __init__(self, bp, part: RowPartition, *, akw: dict, inners, want_q13: bool, group, red_dev, mg_limits, stamp):
        self.bp, self.part, self.akw, self.group, self.red_dev = bp, part, akw, group, red_dev
        self.mg_limits, self.stamp = mg_limits, stamp
        self.n, self.dev = part.n, bp.device
        self.rows = {"u": torch.from_numpy(part.owned_rows(N_VEL_FIELDS).astype(np.int32)).to(self.dev),
                     "p": torch.from_numpy(part.owned_rows(N_P_FIELDS).astype(np.int32)).to(self.dev)}
        self._q_rows = None
        self.op = dict(zip("FDGPQ", self._assemble(inners, want_q13)))

    def _rows_of(self, key):
        return self.rows[_OPS[key][1]]

    def q13_rows(self):
        rows, self._q_rows = self._q_rows, None   # handed over: dead once the diamond is built
        return rows


class _GlobalOperators(_RowSource):
    """Every rank assembles the global F, D, G and forms the global products and multigrid hierarchies (setup memory
    and work O(N) on every rank), then keeps its rows: the only source on one rank, ``local_products=False`` on more."""

    def _assemble(self, inners, want_q13):
        part, n = self.part, self.n
        # (the preconditioner reads F, D and G alone: A's own CSR is not assembled to be dropped)
        _, _, F, D, G = self.bp.get_big_A_matrix(matrix_free_A=n >= 3, **self.akw)
        self.stamp("assemble_global")
        GtG, GtFG = self.bp.commutator_products(F, D, G)
        self.stamp("commutator_products")
        if want_q13:
            blk = np.concatenate([((part.r0 + k) % n) * n + np.arange(n) for k in range(-2, part.L)]).astype(np.int32)
            self._q_rows = self._rows(GtFG, torch.from_numpy(blk).to(self.dev))
        return F, D, G, GtG, GtFG

    def _rows(self, M, rows):
        return M.extract(rows, torch.arange(M.shape[1], dtype=torch.int32, device=self.dev), M.shape[1])

    def resolve(self, ik, key):
        return ik.resolve(self.op[key], self.op[key].diagonal())

    def reach(self, key):
        sub = self._rows(self.op[key], self._rows_of(key))
        return halo_reach(sub.row_ptr, sub.col_idx, self._rows_of(key), self.n)

    def hierarchy(self, ik, key, fields):
        return ik.multigrid(self.op[key], self.n, fields, self.op[key].diagonal())

    def ext_diagonal(self, key, rows):
        return self.op[key].diagonal()[rows.long()].contiguous()

    def owned_ext(self, key, colmap, ncols):
        return self.op[key].extract(self._rows_of(key), colmap, ncols)


class _RankLocalRows(_RowSource):
    """Rank-local setup (preconditioner.py:299-341 row by row): F, D, G assembled on this rank's rows only
    (mpbp_stokes_*_rows, the global assembly's rows bit for bit) and only this rank's pressure rows of Gt_G and Gt_F_G
    (a product's row depends on that row of D alone: the same bits as the global product's row, for a 1 / world share
    of the SpGEMM work); setup memory and work O(N / world + ghosts) instead of O(N).  Needs world > 1."""

    def _assemble(self, inners, want_q13):
        bp, part, n, dev, akw = self.bp, self.part, self.n, self.dev, self.akw
        st_F, st_D, st_G = bp.stencils(**akw)
        F = bp.assemble_rows(_lib.OP_F, self.rows["u"], **akw)
        D = bp.assemble_rows(_lib.OP_D, self.rows["p"], **akw)
        G = bp.assemble_rows(_lib.OP_G, self.rows["u"], **akw)
        F.stencil, D.stencil, G.stencil = st_F, st_D, st_G
        self.stamp("assemble_owned_rows")
        # the products' right operands on the velocity rows a product row can reach -- grid rows within `sup` of the
        # owned ones (the CA schedule's ghost depths included) -- in global row numbering
        sup = min(n, sum(k.sweeps if k.kind in ("jacobi", "chebyshev") else 1 for k in inners) + 2)
        grid_rows = np.unique(np.arange(part.r0 - sup, part.r1 + sup) % n) if part.L + 2 * sup < n else np.arange(n)
        sup_u = np.sort(np.concatenate([f * part.N + (r * n + np.arange(n)) for f in range(N_VEL_FIELDS)
                                        for r in grid_rows]))
        sup_u = torch.from_numpy(sup_u.astype(np.int32)).to(dev)
        Fs = bp.assemble_rows(_lib.OP_F, sup_u, global_shape=True, **akw)
        self.Gs = bp.assemble_rows(_lib.OP_G, sup_u, global_shape=True, **akw)
        self.stamp("assemble_support_rows")
        GtG, GtFG = bp.commutator_products(Fs, D, self.Gs)   # this rank's pressure rows, global columns
        self.stamp("commutator_products")
        GtG.stencil = _gtg_stencil(D, G)
        if want_q13:
            # the two pressure grid rows above the owned block too (their products' rows, bit for bit the global
            # product's), so the symmetric-half read has the lower slots of the first owned rows
            self._q_rows = GtFG
            for k in (1, 2):   # (one grid row per assembly: the wrapped rows need not ascend)
                row = torch.from_numpy((((part.r0 - k) % n) * n + np.arange(n)).astype(np.int32)).to(dev)
                D1 = bp.assemble_rows(_lib.OP_D, row, **akw)
                self._q_rows = _csr_vstack(spgemm(spgemm(D1, Fs, alpha=-1.0), self.Gs, alpha=1.0), self._q_rows)
        return F, D, G, GtG, GtFG

    def resolve(self, ik, key):
        """The Gershgorin bound is the maximum of the ranks' row bounds: the global operator's, exactly, on every rank."""
        import torch.distributed as dist
        M = self.op[key]
        if ik.kind == "chebyshev" and ik.lmax is None:
            t = torch.tensor([M.gershgorin(_row_diagonal(M, self._rows_of(key)))], dtype=torch.float64,
                             device=self.red_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            ik = InnerSolver("chebyshev", ik.sweeps, ik.lmin, float(t.item()), ik.ratio)
        return ik.resolve(M, None)

    def reach(self, key):
        return halo_reach(self.op[key].row_ptr, self.op[key].col_idx, self._rows_of(key), self.n)

    def hierarchy(self, ik, key, fields):
        """This rank's band of level 0 (mg_bands), then its Galerkin levels (LocalHierarchy): no global operator."""
        sizes = level_sizes(self.n, ik.coarsest)
        cap = mg_part_cap(sizes, self.part, len(fields), *self.mg_limits)
        S = mg_bands(sizes, fields, self.part, cap, self.dev)
        self.stamp("mg_bands")
        A0 = self._band(key, S[0])
        self.stamp("mg_band_level0")
        return LocalHierarchy(A0, S, sizes, fields, self.part, self.group, pre=ik.pre, post=ik.post,
                              cycles=int(ik.sweeps), ratio=ik.smooth_ratio, coarsest=ik.coarsest, stamp=self.stamp)

    def _band(self, key, rows, G=None):
        """Rows `rows` of F or of Gt_G = (-D) G, from those rows alone.  G: an assembled G that holds the velocity rows
        those rows of D reach (default: assembled here on exactly them)."""
        if key == "F":
            return self.bp.assemble_rows(_lib.OP_F, rows, **self.akw)
        D = self.bp.assemble_rows(_lib.OP_D, rows, **self.akw)
        if G is None:
            G = self.bp.assemble_rows(_lib.OP_G, torch.unique(D.col_idx), global_shape=True, **self.akw)
        return spgemm(D, G, alpha=-1.0)

    def ext_diagonal(self, key, rows):
        return _row_diagonal(self._band(key, rows, self.Gs), rows)

    def owned_ext(self, key, colmap, ncols):   # already this rank's rows, in owned order
        M = self.op[key]
        return M.extract(torch.arange(M.shape[0], dtype=torch.int32, device=self.dev), colmap, ncols)


def _check_setup_args(inner_F, inner_P, halo, f_mode, pg_mode, ca, layout, numerics):
    """Every refusal that depends on the arguments alone, before any torch.distributed call: a bad argument on one
    rank must not leave the others waiting in a collective."""
    for name, inner in (("inner_F", inner_F), ("inner_P", inner_P)):
        if getattr(inner, "accel", None) is not None:
            raise ValueError(f"{name}: Chebyshev-accelerated multigrid (accel={inner.accel!r}) is not available on "
                             "the row-partitioned hierarchies; use accel=None here")
        if getattr(inner, "coarsen", "even") != "even":
            raise ValueError(f"{name}: coarsen={inner.coarsen!r} is not available under the row partition; use "
                             'coarsen="even" here')
        if getattr(inner, "smoother", "point") != "point":
            raise ValueError(f"{name}: smoother={inner.smoother!r} is one GPU only: the row-partitioned hierarchies "
                             'run the point smoother; use smoother="point" here')
    _check_halo(halo)
    _check_f_mode(f_mode)
    _check_pg_mode(pg_mode)
    _check_layout(layout)
    _check_numerics(numerics)
    if ca not in ("auto", True, False):
        raise ValueError("ca must be 'auto', True or False")
    if ca is True and "mg" in (getattr(inner_F, "kind", None), getattr(inner_P, "kind", None)):
        raise ValueError("ca=True needs Jacobi / Chebyshev inner solves (multigrid exchanges per operator)")


def _split_pieces(M: DeviceCSR, n_own_cols: int, layout: str, split: bool):
    """(the SELL copy or None, _fill_plan's piece) of one operator in the ext layout: its interior rows (no ghost
    column; every row when not `split`) and its boundary rows, as SELL slices of one copy or as CSR row blocks."""
    inner, bnd = boundary_ranges(M.row_ptr, M.col_idx, n_own_cols) if split else ([(0, M.shape[0])], [])
    if layout == "sell":
        S = M.to_sell(inner + bnd)
        n_in = sum((b - a + 63) // 64 for a, b in inner)
        return S, ((None, None), (S.sub(0, n_in), S.sub(n_in, S.nslices - n_in)))
    return None, ((M.plan_blocks(rows=inner) if inner else None, M.plan_blocks(rows=bnd) if bnd else None), (None, None))


class DistributedSchurPreconditioner(PlanProfiling):
    """The approximate-commutator apply over a row partition of the grid (one rank per GPU).

    Every rank forms its rows of the operators (setup only: from its own rows, or from the global operators in its own
    HBM -- ``local_products``), keeps them with columns renumbered into the owned+ghost layout, and runs
    ``mpbp_schur_apply`` with halo callbacks; v and the result hold the rank's owned unknowns [u_n, v_n, u_s, v_s, p]
    rows r0..r1.
    Inner solves: Jacobi / Chebyshev (the communication-avoiding schedule by default) or multigrid ("mg": one
    PartitionedMultigrid per inner inverse, ghost rows exchanged per operator, the coarse levels replicated).

    Graph capture (``capture``) needs the in-order RCCL halo.  A communicator whose exchanges were captured is kept
    until the process exits (``close`` does not destroy it: with RCCL 2.26.6 ncclCommDestroy never returns once a
    graph holding its point-to-point kernels has been instantiated and destroyed; csrc/halo.cpp).
    """

    def __init__(self, n, xi, eta_n, eta_s, c=1.0, d_u=-1.0, inner_F=None, inner_P=None, group=None,
                 device=None, layout="sell", f_mode="auto", pg_mode="auto", halo="auto", self_halo=False,
                 halo_overlap=False, ca="auto", fuse_g=True, mg_min_cells=1 << 14, mg_part_levels=None,
                 local_products=True, numerics="exact", kernel_opts=None):
        _check_setup_args(inner_F, inner_P, halo, f_mode, pg_mode, ca, layout, numerics)
        import torch.distributed as dist
        self.numerics, self.layout = numerics, layout
        # this preconditioner's kernel choices (process defaults now + overrides): tolerance mode reads Gt_F_G's
        # symmetric half over the rank's row block (q13_sym, as one GPU); q13_mf is one-GPU only
        self.kernel_opts = _lib.kernel_opts(kernel_opts)
        # setup phase timings (MPBP_SETUP_TIMING=1: synchronise and stamp each phase; tools/setup_timing.py)
        self.setup_phases = {}
        _stamp = _phase_clock(self.setup_phases)
        self.device = dev = torch.device(device or "cuda")
        # the partition.  self_halo: a single rank still runs the partitioned apply, its ghost rows filled by the
        # periodic self-exchange (exercises the interior / boundary launches and the halo path on one GPU)
        world, backend = dist.get_world_size(group), dist.get_backend(group)
        self.part = part = RowPartition(n, world, dist.get_rank(group), ghosts=bool(self_halo))
        self.partitioned = part.ghosts
        self.halo_impl = halo if halo != "auto" else ("rccl" if backend == "nccl" else "torch")
        red_dev = dev if backend == "nccl" else "cpu"   # where the setup's small all-reduces run
        # the source of this rank's rows; multigrid inner solves form their levels from it too
        ik_f, ik_p = inner_F or InnerSolver(), inner_P or InnerSolver()
        self.local_products = bool(local_products) and world > 1
        src = (_RankLocalRows if self.local_products else _GlobalOperators)(
            MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s, device=dev), part, akw=dict(c=c, d_u=d_u),
            inners=(ik_f, ik_p), want_q13=numerics == "fast" and part.ghosts, group=group, red_dev=red_dev,
            mg_limits=(mg_min_cells, mg_part_levels), stamp=_stamp)
        self._decide_q13(src.q13_rows(), group, red_dev)
        self.f_stencil = _f_stencil(src.op["F"], f_mode)
        self.pg_stencil = _pg_stencil(src.op["D"], src.op["G"], src.op["P"], self.f_stencil, pg_mode)
        # inner-solver bounds from the global operators: identical on every rank
        self.inner_F = src.resolve(ik_f, "F")
        self.inner_P = src.resolve(ik_p, "P")
        mg_any = "mg" in (self.inner_F.kind, self.inner_P.kind)
        _stamp("inner_bounds")
        q = src.reach("Q")
        self.h_u = max(1, src.reach("F"), src.reach("D"))
        self.h_p = max(1, src.reach("G"), src.reach("P"), q)
        # multigrid inner solves: the hierarchies split over the partition; level 0's ghost layout must also serve the
        # restriction's reach
        self.mg_F = self.mg_P = None
        kw = dict(group=group, min_cells=mg_min_cells, max_part_levels=mg_part_levels)
        if self.inner_F.kind == "mg":
            gF = src.hierarchy(self.inner_F, "F", FIELDS_VELOCITY)
            self.mg_F = PartitionedMultigrid(gF, part, N_VEL_FIELDS, **kw) if self.partitioned else gF
        if self.inner_P.kind == "mg":
            gP = src.hierarchy(self.inner_P, "P", FIELDS_PRESSURE)
            self.mg_P = PartitionedMultigrid(gP, part, N_P_FIELDS, **kw) if self.partitioned else gP
        if isinstance(self.mg_F, PartitionedMultigrid):
            self.h_u = max(self.h_u, self.mg_F.h0)
        if isinstance(self.mg_P, PartitionedMultigrid):
            self.h_p = max(self.h_p, self.mg_P.h0)
        _stamp("halo_reach_and_multigrid")
        self._ca_depths(ca, mg_any, q)
        # CA schedule: the second F solve recomputes G x_p inside its sweeps from x_p's ghost rows (no G launch)
        self.fuse_g = bool(fuse_g and self.ca and self.inner_F.kind == "chebyshev" and self.inner_F.sweeps >= 2)
        if self.ca:   # diagonals on owned + ghost rows (the CA schedule's ghost-row sweeps stage x0)
            self.diag_F_ext, self.diag_P_ext = (
                src.ext_diagonal(key, torch.from_numpy(part.ext_rows(nf, h).astype(np.int32)).to(dev))
                for key, nf, h in (("F", N_VEL_FIELDS, self.h_u), ("P", N_P_FIELDS, self.h_p)))
        _stamp("ca_ghost_diagonals")
        # the ext layout: every operator's owned rows, columns renumbered into owned + ghost slots
        self.nu, self.np = part.n_owned(N_VEL_FIELDS), part.n_owned(N_P_FIELDS)
        self.nu_ext, self.np_ext = part.n_ext(N_VEL_FIELDS, self.h_u), part.n_ext(N_P_FIELDS, self.h_p)
        self.shape = (self.nu + self.np, self.nu + self.np)
        ext = {"u": (torch.from_numpy(part.colmap(N_VEL_FIELDS, self.h_u)).to(dev), self.nu_ext),
               "p": (torch.from_numpy(part.colmap(N_P_FIELDS, self.h_p)).to(dev), self.np_ext)}
        for key, (attr, _, cols) in _OPS.items():
            setattr(self, attr, src.owned_ext(key, *ext[cols]))
        del src
        torch.cuda.empty_cache()
        self.diag_F = self.F.diagonal()
        self.diag_P = self.GtG.diagonal()
        _stamp("extract_ghost_layout")
        own_cols = {"u": self.nu, "p": self.np}
        self._sells, self._pieces = {}, {}
        for key, (attr, _, cols) in _OPS.items():
            self._sells[key], self._pieces[key] = _split_pieces(getattr(self, attr), own_cols[cols], layout, world > 1)
        _stamp("sell_layouts")
        self._workspace_and_halos(group, halo_overlap, _stamp)
        _stamp("halo_and_workspace")
        self._prof = None
        self._plan = self._make_plan()
        _stamp("plan")

    def _decide_q13(self, q_rows, group, red_dev):
        """Fast numerics: Gt_F_G's diamond over the rank's row block (self.q13), read from its symmetric upper half
        (k_q13p; kernel option q13_sym) when the product is symmetric to 1e-14 of its largest entry -- decided over all
        ranks, as one GPU decides over the whole grid.  q_rows: the source's q13_rows()."""
        self.q13 = None
        if q_rows is not None and self.part.n >= 5:
            self.q13 = _q13_block(q_rows, self.part.n, self.part, group, red_dev)
        if self.q13 is None or not self.q13[2]:
            self.kernel_opts.q13_sym = 0

    def _ca_depths(self, ca, mg_any: bool, q: int):
        """The communication-avoiding schedule (mpbp_schur_plan.ca): v's halo and x_b's halo only, deep enough for
        every matrix-free operator to also compute the ghost rows its successors read.  Sets ca and ca_q (Gt_F_G's
        reach) and deepens h_u / h_p when the schedule is taken; ca=True raises where it cannot be."""
        part = self.part
        self.ca, self.ca_q = False, q
        if ca and not mg_any and part.ghosts and self.f_stencil is not None and self.pg_stencil is not None:
            sf, sp = self.inner_F.sweeps - 1, self.inner_P.sweeps - 1
            hu, hp = q + sp + 1 + sf, max(q + sp, sf + 1 + sp, q)
            if max(hu, hp) <= part.min_rows:
                self.ca = True
                self.h_u, self.h_p = max(self.h_u, hu), max(self.h_p, hp)
            elif ca is True:
                raise ValueError(f"ca=True needs {max(hu, hp)} grid rows per rank, the smallest has {part.min_rows}")
        elif ca is True:
            raise ValueError("ca=True needs a row partition and the matrix-free F, D, G, Gt_G")

    def _workspace_and_halos(self, group, halo_overlap: bool, stamp):
        """The apply's work vectors (ext layout) and, under a partition, the exchanges of their ghost rows: the RCCL
        halo object or the host-staged kinds, and each partitioned multigrid hierarchy built on them -- its level 0 is
        the apply's own F / Gt_G with the apply's ping / pong buffers."""
        part, dev = self.part, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        self._wu = [torch.zeros(self.nu_ext, **f64) for _ in range(4)]
        self._wu_owned = torch.zeros(self.nu, **f64)
        self._wp = [torch.zeros(self.np_ext, **f64) for _ in range(7)]
        self._wu_ext = torch.zeros(self.nu_ext if self.ca else 0, **f64)
        self._rccl = self._halos = None
        if not self.partitioned:
            return
        if self.halo_impl == "rccl":
            self._rccl = RcclHalo(part, self.h_u, self.h_p, group, overlap=halo_overlap)
        self._halos = _Halos(self.halo_impl, self._rccl, group, dev)
        if self._rccl is None:
            self._halos.add_kind(part, N_VEL_FIELDS, self.h_u, kind=_lib.VEC_VELOCITY)
            self._halos.add_kind(part, N_P_FIELDS, self.h_p, kind=_lib.VEC_PRESSURE)
        self._halos.register(*self._wu, *self._wp, *([self._wu_ext] if self.ca else []))
        if isinstance(self.mg_F, PartitionedMultigrid):
            self.mg_F.build(self._halos, (self._wu[1], self._wu[2]), self.diag_F, self.h_u, kind0=_lib.VEC_VELOCITY)
            stamp("mg_build_F")
        if isinstance(self.mg_P, PartitionedMultigrid):
            self.mg_P.build(self._halos, (self._wp[4], self._wp[5]), self.diag_P, self.h_p, kind0=_lib.VEC_PRESSURE)
            stamp("mg_build_P")

    def _make_plan(self):
        p = _fill_plan(self, self._pieces)
        # velocity (F, D) and pressure (G, Gt_G) input partitions of the stencil operators
        ghost = self.partitioned
        p.f_part = _lib.RowPart(self.part.r0, self.part.L, self.h_u if ghost else 0, 0)
        p.p_part = _lib.RowPart(self.part.r0, self.part.L, self.h_p if ghost else 0, 0)
        p.halo = self._halos.fn if self._halos is not None else _lib.HALO_FN()
        p.halo_ctx = self._rccl.handle if self._rccl is not None else None
        # the in-order RCCL schedule gains nothing from splitting rows around the exchange: exchange first,
        # then one launch per sweep
        p.halo_first = 1 if (self._rccl is not None and not self._rccl.overlap) else 0
        p.ca, p.ca_reach_q = (1 if self.ca else 0), self.ca_q
        if self.ca:
            if self._rccl is not None and not self._rccl.overlap:   # v's two halves in one RCCL group
                p.halo_pair = self._rccl.pair_fn
            p.wu_ext = self._wu_ext.data_ptr()
            p.diag_F_ext, p.diag_P_ext = self.diag_F_ext.data_ptr(), self.diag_P_ext.data_ptr()
        return p

    def sell_of(self, key):
        """The SELL-64 copy (interior + boundary slices) of F / D / G / P / Q, or None (CSR layout)."""
        return self._sells[key]

    def apply(self, v: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        assert v.is_cuda and v.dtype == torch.float64 and v.numel() == self.nu + self.np
        if out is None:
            out = torch.empty_like(v)
        check(lib().mpbp_schur_apply(ctypes.byref(self._plan), ptr(v), ptr(out), stream_handle()))
        # every exchange and gather of the apply (its own halos and the partitioned multigrid levels') reports through
        # _Halos: the RCCL object's status, or the first exception a host-staged callback latched
        if self._halos is not None:
            self._halos.check()
        return out

    def capture(self, v: torch.Tensor, out: torch.Tensor):
        """Capture one apply(v, out) into a hipGraph.  Partitioned applies need the RCCL halo in order on the
        apply stream (the exchange is then a gather kernel plus one RCCL group of point-to-point calls, which
        RCCL records into the graph); the capture runs in thread-local error mode so that RCCL's proxy thread
        may keep calling HIP.  The torch halo (host-staged gloo collectives between kernels) cannot be
        captured."""
        if self.partitioned and (self._rccl is None or self._rccl.overlap):
            raise NotImplementedError("graph capture of a partitioned apply needs the in-order RCCL halo")
        return _capture(self, v, out, capture_error_mode="thread_local" if self.partitioned else "global")

    def close(self):
        if self._rccl is not None:
            self._rccl.close()
            self._rccl = None

    def local_to_global_rows(self):
        """Global ids (in the [u_n, v_n, u_s, v_s, p] numbering) of this rank's v / out entries."""
        return np.concatenate([self.part.owned_rows(N_VEL_FIELDS),
                               4 * self.part.N + self.part.owned_rows(N_P_FIELDS)])


def solve_distributed(n, xi, etan, etas, c=1.0, d=-1.0, b_vec=None, inner_F=None, inner_P=None, tol=1e-8,
                      maxiter=150, restrt=None, group=None, self_halo=False, keep_operators=False,
                      matrix_free_A=False, **pc_kw):
    """solve.py:240-286 over a row partition (one rank per GPU): FGMRES (solve.fgmres over `group`) on the partitioned
    operator A (DistributedMatrix) with the partitioned approximate-commutator preconditioner
    (DistributedSchurPreconditioner).  b_vec: the global right-hand side on the host (default: the manufactured problem
    of solve.py:52-80).  The solve is the one-GPU solve's, bit for bit (reproducible inner products).  Returns a dict:
    x_local (this rank's rows of the iterate, CUDA), rows (their global ids), info, residuals, A, M.  Unless
    keep_operators, A and M are closed before the return (their RCCL communicators destroyed here, at the same point on
    every rank, also when the solve raises -- not whenever the garbage collector of each rank gets to them).
    matrix_free_A: the operator is a DistributedStokesOperator over ``bp.stokes_operator(c, d)`` (exact numerics) -- no
    row of A is assembled on any rank, at any world size (self_halo included; n >= 3); its rows are the assembled ones
    bit for bit, so the iterates and the residual history are the same."""
    import torch.distributed as dist
    from .preconditioner import MultiphaseBlockPreconditioner
    from .solve import fgmres
    from .utils import manufactured_problem
    bp = MultiphaseBlockPreconditioner(n, xi, etan, etas)
    world = dist.get_world_size(group)
    if matrix_free_A:
        dA = DistributedStokesOperator(bp.stokes_operator(c, d), group=group, self_halo=self_halo,
                                       halo=pc_kw.get("halo", "auto"))
    elif world > 1:   # rank-local: this rank's rows of A only
        part = RowPartition(n, world, dist.get_rank(group))
        rows = torch.from_numpy(part.owned_rows(5).astype(np.int32)).cuda()
        dA = DistributedMatrix(bp.assemble_rows(_lib.OP_A, rows, c=c, d_u=d), n, 5, group=group, owned_rows=True,
                               halo=pc_kw.get("halo", "auto"))
    else:
        dA = DistributedMatrix(bp.get_big_A_matrix(c=c, d_u=d)[0], n, 5, group=group, self_halo=self_halo,
                               halo=pc_kw.get("halo", "auto"))
    del bp
    torch.cuda.empty_cache()
    M = None
    try:
        M = DistributedSchurPreconditioner(n, xi, etan, etas, c=c, d_u=d, inner_F=inner_F, inner_P=inner_P,
                                           group=group, self_halo=self_halo, **pc_kw)
        if b_vec is None:
            _, b_vec = manufactured_problem(n, c, d, xi, etan, etas)
        rows = dA.local_to_global_rows()
        assert np.array_equal(rows, M.local_to_global_rows())
        b = torch.from_numpy(np.ascontiguousarray(np.asarray(b_vec, dtype=np.float64)[rows])).cuda()
        kgroup = (group if group is not None else dist.group.WORLD) if world > 1 else None
        hist = []
        x, info = fgmres(dA, b, M=M, tol=tol, maxiter=maxiter, restrt=restrt, residuals=hist, group=kgroup)
        torch.cuda.synchronize()
    finally:
        if not keep_operators:
            dA.close()
            if M is not None:
                M.close()
    return {"x_local": x, "rows": rows, "info": info, "residuals": hist, "A": dA, "M": M}
