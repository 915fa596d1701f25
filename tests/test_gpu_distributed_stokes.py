"""The matrix-free system matrix under the row partition (DistributedStokesOperator, mpbp_stokes_apply_part): every
rank's rows of A u recomputed from the thn tables, bit for bit the rows of the assembled A's CSR product and of the
one-GPU StokesOperator (exact numerics) or of the one-GPU fast operator (fast numerics).  gloo ranks share one GPU (the
pattern of test_gpu_distributed.py); the RCCL halo kind runs as the periodic self-exchange, and between two GPUs where
the node has them.  Each spawn loops over its cases, so the file costs a handful of process launches."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# (xi, eta_n, eta_s, c, d_u, d_p, d_div): the reference's parameters (every compile-time identity of the F policy
# taken), general ones (none taken), and c = 0 with eta_n = 1 -- the sets of test_gpu_stokes_operator.py
PARAMS = {"visc": (1.0, 100.0, 1.0, 1.0, -1.0, 1.0, -1.0), "general": (2.5, 1.0e4, 1.0, 0.5, -2.0, 0.5, -2.0),
          "c0": (1.0, 1.0, 1.0, 0.0, -1.0, 1.0, -1.0)}
STORE, ADD, RESID, FAST = 0, 1, 2, 0x100
SENTINEL = -7.25


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, args, nprocs, errfile):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    try:
        mp.spawn(fn, args=args, nprocs=nprocs, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")


def _init(rank, world, port, backend="gloo", device=0):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(device)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)


def _raw(dA, which, mode, z, out):
    """mpbp_stokes_apply_part on dA's ext buffer (ghost rows as the last apply left them)."""
    from mp_block_preconditioners_amd import _lib
    from mp_block_preconditioners_amd._lib import check, lib, ptr, stream_handle
    op, part = dA.op, dA.part
    rp = _lib.RowPart(part.r0, part.L, dA.h, which, 0, 0)
    flags = mode | (FAST if op.numerics == "fast" else 0)
    check(lib().mpbp_stokes_apply_part(ctypes.byref(op.prm), ptr(op.cell), ptr(op.uface), ptr(op.vface),
                                       ctypes.byref(rp), flags, ptr(dA.xe), ptr(z), ptr(out), stream_handle()))
    return out


def _check_case(n, world, dev="cuda", halo="auto", overlap=True, self_halo=False, march=(0,)):
    """Every parameter set at one (world, n): the partitioned operator's rows against the one-GPU operators' rows."""
    import mp_block_preconditioners_amd as mpb
    from mp_block_preconditioners_amd._lib import kernel_options
    from mp_block_preconditioners_amd.distributed import DistributedStokesOperator
    assert mpb.DistributedStokesOperator is DistributedStokesOperator
    rng = np.random.default_rng(100 + n)
    us = [torch.from_numpy(rng.standard_normal(5 * n * n)).to(dev) for _ in range(3)]
    zg = torch.from_numpy(rng.standard_normal(5 * n * n)).to(dev)
    dAs = {}   # one partitioned operator per numerics: the later parameter sets reach it through set_params
    for name, (xi, eta_n, eta_s, c, d_u, d_p, d_div) in PARAMS.items():
        kw = dict(c=c, d_u=d_u, d_p=d_p, d_div=d_div)
        bp = mpb.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s, device=dev)
        A = bp.get_big_A_matrix(**kw)[0]
        ops = {num: bp.stokes_operator(numerics=num, **kw) for num in ("exact", "fast")}
        refs = {num: [ops[num].matvec(u) for u in us] for num in ops}
        csr = [A.matvec(u) for u in us]
        for num, op in ops.items():
            if num not in dAs:
                held = bp.stokes_operator(numerics=num, **kw)
                dAs[num] = DistributedStokesOperator(held, halo=halo, overlap=overlap, self_halo=self_halo)
                assert dAs[num].op is held
            dA = dAs[num]
            dA.op.set_params(xi=xi, eta_n=eta_n, eta_s=eta_s, **kw)
            part = dA.part
            assert dA.partitioned and dA.nfields == 5 and dA.h == 1 and dA.numerics == num
            assert dA.n_own == 5 * part.L * n and dA.n_ext == 5 * (part.L + 2) * n and dA.shape == (dA.n_own,) * 2
            assert dA.halo_impl == ("torch" if halo == "auto" else halo) and dA.device == op.device
            gids = torch.from_numpy(dA.local_to_global_rows()).to(dev)
            assert gids.numel() == dA.n_own
            tag = (name, num, world, n)
            for rows in march:
                with kernel_options(march_rows=rows):
                    for k, u in enumerate(us):   # three different vectors: a stale ghost row would show
                        got = dA.apply(u[gids].contiguous())
                        assert torch.equal(got, refs[num][k][gids]), (tag, rows, k)
                        if num == "exact":
                            assert torch.equal(got, csr[k][gids]), (tag, rows, k)
                    # the three epilogues through the raw entry; the ext buffer holds us[-1] with its ghost rows
                    z = zg[gids].contiguous()
                    for mode in (STORE, ADD, RESID):
                        want = (A.matvec(us[-1], mode=mode, z=zg) if num == "exact"
                                else op.matvec(us[-1], mode=mode, z=zg))[gids]
                        whole = _raw(dA, 0, mode, z, torch.full_like(z, SENTINEL))
                        assert torch.equal(whole, want), (tag, rows, mode)
                        split = torch.full_like(z, SENTINEL)   # interior then the two edge rows: every row once
                        _raw(dA, 1, mode, z, split)
                        if part.L <= 2:
                            assert bool((split == SENTINEL).all()), (tag, "empty interior")
                        _raw(dA, 2, mode, z, split)
                        assert torch.equal(split, want), (tag, rows, mode)
            out = torch.full((dA.n_own,), SENTINEL, dtype=torch.float64, device=dev)
            assert dA.matvec(us[0][gids].contiguous(), out=out) is out and torch.equal(out, refs[num][0][gids])
    for dA in dAs.values():
        dA.close()


def _bits_worker(rank, world, port, cases, errfile):
    try:
        _init(rank, world, port)
        for n, march in cases:
            _check_case(n, world, march=march)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {type(e).__name__}: {e!r}\n")
        raise


MARCH = (0, 1, 3, 8)


@pytest.mark.parametrize("world,cases", [
    (3, ((3, (0,)), (50, (0,)), (257, MARCH))),   # one grid row per rank (every row an edge row, empty interior,
                                                  # both ghosts from different ranks); two strips, uneven rows
    (4, ((9, (0,)),)),                            # the uneven split 3 / 2 / 2 / 2
    (2, ((5, (0,)), (64, MARCH))),
], ids=["world3", "world4", "world2"])
def test_partitioned_rows_bits(world, cases, tmp_path):
    """Exact numerics: the rows of the assembled A's CSR product and of the one-GPU StokesOperator, bit for bit; fast
    numerics: the one-GPU fast operator's rows bit for bit; STORE / ADD / RESID through mpbp_stokes_apply_part."""
    errfile = str(tmp_path / "err.txt")
    _spawn(_bits_worker, (world, _free_port(), cases, errfile), world, errfile)


def _self_halo_worker(_index, port, n, halo, overlap, errfile):
    try:
        _init(0, 1, port)
        _check_case(n, 1, halo=halo, overlap=overlap, self_halo=True)
        if halo == "torch":   # unpartitioned: the one-GPU operator itself
            import mp_block_preconditioners_amd as mpb
            bp = mpb.MultiphaseBlockPreconditioner(8, 1.0, 100.0, 1.0)
            op = bp.stokes_operator(1.0, -1.0)
            dA = mpb.DistributedStokesOperator(op)
            assert not dA.partitioned and dA.n_own == dA.n_ext == 5 * 64
            u = torch.from_numpy(np.random.default_rng(0).standard_normal(5 * 64)).cuda()
            assert torch.equal(dA.apply(u), op.matvec(u))
            dA.close()
        dist.destroy_process_group()
    except BaseException as e:
        with open(errfile, "a") as f:
            f.write(f"{type(e).__name__}: {e!r}\n")
        raise


@pytest.mark.parametrize("n,halo,overlap", [(3, "torch", True), (64, "rccl", True), (64, "rccl", False),
                                            (33, "rccl", True), (33, "rccl", False)])
def test_self_halo_rows_bits(n, halo, overlap, tmp_path):
    """One rank exchanging with itself (the periodic wrap): the torch halo at n = 3, the RCCL kind overlapped on the
    halo's side stream and in order at n = 64 and 33."""
    errfile = str(tmp_path / "err.txt")
    _spawn(_self_halo_worker, (_free_port(), n, halo, overlap, errfile), 1, errfile)


def _shifted_tables(n):
    """Another smooth field, 0.5 + 0.3 cos(2 pi (x + 0.1)) sin(4 pi (y - 0.2)), at the three tables' points."""
    r, c = np.divmod(np.arange(n * n), n)
    dx = 1.0 / n

    def f(y, x):
        return 0.5 + 0.3 * np.cos(2 * np.pi * (x + 0.1)) * np.sin(4 * np.pi * (y - 0.2))
    return f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx)


def _time_step_worker(rank, world, port, n, errfile):
    try:
        _init(rank, world, port)
        import mp_block_preconditioners_amd as mpb
        bp = mpb.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0)
        op = bp.stokes_operator(c=1.0, d_u=-1.0)
        dA = mpb.DistributedStokesOperator(op)
        gids = torch.from_numpy(dA.local_to_global_rows()).cuda()
        u = torch.from_numpy(np.random.default_rng(5).standard_normal(5 * n * n)).cuda()
        before = dA.apply(u[gids].contiguous())
        assert torch.equal(before, bp.get_big_A_matrix(c=1.0, d_u=-1.0)[0].matvec(u)[gids])
        xe = dA.xe.data_ptr()
        bp.update_theta_tables(*_shifted_tables(n))
        bp.xi, bp.eta_n, bp.eta_s = 2.5, 40.0, 3.0
        new = dict(c=0.5, d_u=-2.0, d_p=0.5, d_div=-2.0)
        op.set_params(xi=bp.xi, eta_n=bp.eta_n, eta_s=bp.eta_s, **new)
        fresh = bp.get_big_A_matrix(**new)[0]
        got = dA.apply(u[gids].contiguous())
        assert dA.xe.data_ptr() == xe and not hasattr(dA, "refill")
        assert torch.equal(got, fresh.matvec(u)[gids])
        assert not torch.equal(got, before)
        dA.close()
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {type(e).__name__}: {e!r}\n")
        raise


def test_time_step(tmp_path):
    """New thn values (update_theta_tables) and new xi, eta, c, d_u, d_p, d_div (set_params) reach the same
    DistributedStokesOperator object with no rebuild: it equals a freshly assembled A's rows bit for bit."""
    errfile = str(tmp_path / "err.txt")
    _spawn(_time_step_worker, (2, _free_port(), 24, errfile), 2, errfile)


CHEB = (("chebyshev", 4), ("chebyshev", 4))
MG1 = (("mg", 1), ("mg", 1))


def _solve_worker(rank, world, port, n, errfile):
    try:
        _init(rank, world, port)
        import mp_block_preconditioners_amd as mpb
        from mp_block_preconditioners_amd import _lib
        from mp_block_preconditioners_amd.distributed import (DistributedMatrix, DistributedStokesOperator,
                                                              solve_distributed)
        # which operators the solve assembles (whole, or by rows): A must not be among them when matrix-free
        seen = []
        cls = mpb.MultiphaseBlockPreconditioner
        whole, by_rows = cls.assemble, cls.assemble_rows

        def assemble(self, op, *a, **k):
            seen.append(int(op))
            return whole(self, op, *a, **k)

        def assemble_rows(self, op, *a, **k):
            seen.append(int(op))
            return by_rows(self, op, *a, **k)
        cls.assemble, cls.assemble_rows = assemble, assemble_rows
        for inner, maxiter in ((CHEB, 40), (MG1, 60)):
            runs = []
            for mf in (False, True):
                del seen[:]
                iF, iP = (mpb.InnerSolver(*s) for s in inner)
                res = solve_distributed(n, 1.0, 100.0, 1.0, inner_F=iF, inner_P=iP, tol=1e-8, maxiter=maxiter,
                                        mg_min_cells=0, self_halo=(world == 1), matrix_free_A=mf)
                assert (_lib.OP_A in seen) == (not mf), (mf, seen)
                runs.append(res)
            a, m = runs
            assert isinstance(a["A"], DistributedMatrix) and isinstance(m["A"], DistributedStokesOperator)
            assert m["A"].partitioned and a["A"].partitioned
            held = [k for k, v in vars(m["A"]).items() if isinstance(v, (mpb.DeviceCSR, _lib.RowBlocks))]
            assert not held and not hasattr(m["A"], "A") and not hasattr(m["A"], "blk_in"), held
            assert a["info"] == m["info"] and a["residuals"] == m["residuals"] and len(m["residuals"]) > 1
            assert np.array_equal(a["rows"], m["rows"]) and torch.equal(a["x_local"], m["x_local"])
            if inner is MG1:
                assert m["info"] == 0
        cls.assemble, cls.assemble_rows = whole, by_rows
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {type(e).__name__}: {e!r}\n")
        raise


@pytest.mark.parametrize("world", [2, 1], ids=["world2", "self_halo"])
def test_solve_matrix_free_A(world, tmp_path):
    """solve_distributed(matrix_free_A=True) against matrix_free_A=False: the same info, residual history and iterate
    bit for bit (Chebyshev and multigrid inner solves), the operator a DistributedStokesOperator holding no CSR arrays,
    and no assembly call for A on any rank; world 1 runs the periodic self-exchange."""
    errfile = str(tmp_path / "err.txt")
    _spawn(_solve_worker, (world, _free_port(), 32, errfile), world, errfile)


def _rccl_worker(rank, world, port, n, errfile):
    try:
        _init(rank, world, port, backend="nccl", device=rank)
        _check_case(n, world, dev=f"cuda:{rank}", halo="rccl")
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {type(e).__name__}: {e!r}\n")
        raise


def test_rccl_two_gpus_rows_bits(tmp_path):
    """The partitioned operator over RCCL point-to-point between two GPUs (one rank per GPU), bit for bit against the
    one-GPU operators.  Runs where the node has two GPUs; skipped on a one-GPU box."""
    world, n = 2, 130
    if not torch.cuda.is_available() or torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs")
    errfile = str(tmp_path / "err.txt")
    _spawn(_rccl_worker, (world, _free_port(), n, errfile), world, errfile)
