"""A u three ways at one grid size: the assembled A's CSR product (the yardstick), the matrix-free StokesOperator
with exact numerics and with fast numerics; then the same FGMRES solve with the assembled A and with the exact
operator, and the device memory with and without A assembled.

    python tools/stokes_apply_timing.py [--n 1024] [--launches 200] [--rounds 5] [--out profiles/stokes_operator_timing_1024.json]

Kernel timing: one device-event pair around `launches` back-to-back launches of a contender (captured into a graph, so
the host's launch rate is not in the figure), after a warm replay; the three contenders alternate in the same process
for `rounds` rounds; min-max microseconds per launch over the rounds.
Algorithmic bytes: matrix-free 104 B per cell (5 fields read, 5 written, 3 thn tables); CSR as bench.py counts it
(12 B per entry, x and y, the row blocks' wave table).  Solve: fgmres to 1e-8 on the manufactured problem with
InnerSolver("mg", 6, accel="chebyshev") / InnerSolver("mg", 1), fast numerics, the apply's graph captured beforehand;
the iteration counts of the two runs must be equal.

    python tools/stokes_apply_timing.py --partitioned [--n 1024] [--out profiles/stokes_partitioned_timing_1024.json]

The same operator under the row partition, in ONE process exchanging ghost rows with itself over RCCL (self_halo: the
periodic wrap; a one-GPU self-exchange, not an xGMI transfer between GPUs): DistributedMatrix.apply on the assembled A
against DistributedStokesOperator.apply with exact and fast numerics, overlap on and off.  A partitioned apply is a
copy, an exchange and two launches issued from the host, so it is timed eagerly: one device-event pair around
`launches` back-to-back applies (the host's issue rate is part of the figure, equally for every contender), after
`launches` warm applies; the contenders alternate for `rounds` rounds.  Also the allocated device memory of either
operator, and the one-GPU StokesOperator graph-timed as above in the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def csr_bytes(A):
    """bench.py's algorithmic bytes of one CSR product of A."""
    import numpy as np
    t = A.blocks.table.cpu().numpy().reshape(-1, 8).astype(np.int64)
    nonuni = 0
    for w in range(4):
        rows_w = np.clip(t[:, 1] - (t[:, 0] + 64 * w), 0, 64)
        nonuni += int(rows_w[((t[:, 7] >> (8 * w)) & 255) == 0].sum())
    struct = A.blocks.count * 32 + (nonuni * 4 + A.blocks.count * 8 if nonuni else 0)
    return A.nnz * 12 + (A.shape[0] + A.shape[1]) * 8 + struct


def _graph_time(contenders, x, y, launches, rounds):
    """{name: [us per launch, per round]}: each contender's `launches` back-to-back launches captured into a graph and
    replayed between a device-event pair after a warm replay, the contenders alternating per round."""
    import torch
    us = {name: [] for name, _ in contenders}
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name, fn in contenders:
            fn(x, out=y)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(launches):
                    fn(x, out=y)
            graphs[name] = g
    torch.cuda.current_stream().wait_stream(side)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for name, _ in contenders:
            graphs[name].replay()
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    return us


def _spread(v):
    return {"us_min": min(v), "us_max": max(v), "us_rounds": v}


def partitioned(a):
    """The --partitioned case (module docstring)."""
    import socket

    import torch
    import torch.distributed as dist

    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd.distributed import DistributedMatrix, DistributedStokesOperator

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    n, N = a.n, a.n * a.n
    xi, eta_n, eta_s, c, d_u = 1.0, a.eta_n, 1.0, 1.0, -1.0

    def allocated():
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()
    base = allocated()
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    ops = {num: bp.stokes_operator(c=c, d_u=d_u, numerics=num) for num in ("exact", "fast")}
    mem_tables = allocated() - base
    x = torch.randn(5 * N, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.empty_like(x)
    one_gpu = _graph_time([(num, op.matvec) for num, op in ops.items()], x, y, a.launches, a.rounds)
    res = {"n": n, "eta_n": eta_n, "launches_per_round": a.launches, "rounds": a.rounds,
           "one_gpu_stokes_operator": {"timing": "graph replay of the back-to-back launches between a device-event pair",
                                       **{num: _spread(v) for num, v in one_gpu.items()}},
           "partitioned": {"world": 1, "halo": "rccl self-exchange on one GPU (the periodic wrap): not an xGMI "
                                               "measurement; no multi-GPU hardware run exists",
                           "timing": "one device-event pair around the back-to-back eager applies (copy, exchange, two "
                                     "launches each; the host's issue rate included), after as many warm applies; "
                                     "contenders alternate per round"}}
    recorded = os.path.join(ROOT, "profiles", f"stokes_operator_timing_{n}.json")
    if os.path.exists(recorded):   # the figures this tool gave when the one-GPU operator was merged (same method)
        with open(recorded) as f:
            k = json.load(f)["kernels"]
        res["one_gpu_stokes_operator"]["recorded_at_merge"] = {
            num: {"us_min": k[num]["us_min"], "us_max": k[num]["us_max"]} for num in ("exact", "fast")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for overlap in (True, False):
        before = allocated()
        A = bp.assemble(0, c=c, d_u=d_u)
        dM = DistributedMatrix(A, n, 5, halo="rccl", overlap=overlap, self_halo=True)
        del A
        torch.cuda.empty_cache()
        mem_csr = allocated() - before
        before = allocated()
        dS = {num: DistributedStokesOperator(op, halo="rccl", overlap=overlap, self_halo=True) for num, op in ops.items()}
        mem_mf = (allocated() - before) // len(dS)
        contenders = [("csr", dM)] + [(num, d) for num, d in dS.items()]
        ref = dM.apply(x).clone()
        assert torch.equal(dS["exact"].apply(x), ref), "the exact partitioned operator must equal the CSR rows bit for bit"
        assert torch.equal(ref, ops["exact"].matvec(x))
        fast_err = float((dS["fast"].apply(x) - ref).abs().max() / ref.abs().max())
        us = {name: [] for name, _ in contenders}
        for _ in range(a.rounds):
            for name, d in contenders:
                for _ in range(a.launches):
                    d.apply(x, out=y)
                e0.record()
                for _ in range(a.launches):
                    d.apply(x, out=y)
                e1.record()
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        for _, d in contenders:
            d.close()
        del dM, dS, contenders
        torch.cuda.empty_cache()
        res["partitioned"]["overlap" if overlap else "in_order"] = {
            **{name: _spread(v) for name, v in us.items()},
            "fast_rel_inf_vs_csr": fast_err,
            "csr_over_exact": [min(us["csr"]) / max(us["exact"]), max(us["csr"]) / min(us["exact"])],
            "csr_over_fast": [min(us["csr"]) / max(us["fast"]), max(us["csr"]) / min(us["fast"])],
            "memory_bytes": {"assembled_rows_ext_buffer_and_row_blocks": mem_csr,
                             "matrix_free_ext_buffer": mem_mf, "thn_tables_shared_by_both_numerics": mem_tables}}
    dist.destroy_process_group()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eta-n", type=float, default=100.0)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--partitioned", action="store_true", help="the row-partitioned operators over the RCCL self-exchange")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 1 or a.rounds < 1:
        ap.error("--launches and --rounds must be positive")
    if a.partitioned:
        res = partitioned(a)
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        return
    import numpy as np
    import torch

    import mp_block_preconditioners_amd as mp

    n, N = a.n, a.n * a.n
    xi, eta_n, eta_s, c, d_u = 1.0, a.eta_n, 1.0, 1.0, -1.0
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
    op, _, F, D, G = bp.get_big_A_matrix(c=c, d_u=d_u, matrix_free_A=True)
    torch.cuda.synchronize()
    mem_free = torch.cuda.memory_allocated() - base
    A = bp.assemble(0, c=c, d_u=d_u)
    A.row_groups = 5
    A.blocks
    torch.cuda.synchronize()
    mem_A = torch.cuda.memory_allocated() - base - mem_free
    fast = bp.stokes_operator(c=c, d_u=d_u, numerics="fast")

    x = torch.randn(5 * N, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    y = torch.empty_like(x)
    contenders = (("csr", A.matvec, csr_bytes(A)), ("exact", op.matvec, 104 * N), ("fast", fast.matvec, 104 * N))
    ref = A.matvec(x).clone()
    assert torch.equal(op.matvec(x), ref), "the exact operator must equal the CSR product bit for bit"
    fast_err = float((fast.matvec(x) - ref).abs().max() / ref.abs().max())
    us = {name: [] for name, _, _ in contenders}
    graphs = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for name, fn, _ in contenders:   # `launches` back-to-back launches per graph: no host launch rate in the timing
            fn(x, out=y)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(a.launches):
                    fn(x, out=y)
            graphs[name] = g
    torch.cuda.current_stream().wait_stream(side)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, _, _ in contenders:
            graphs[name].replay()        # warm-up: `launches` launches
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    kernels = {}
    for name, _, nbytes in contenders:
        lo, hi = min(us[name]), max(us[name])
        kernels[name] = {"us_min": lo, "us_max": hi, "us_rounds": us[name], "algorithmic_bytes": nbytes,
                         "gbs_at_min": nbytes / lo / 1e3, "gbs_at_max": nbytes / hi / 1e3}
    res = {"n": n, "eta_n": eta_n, "launches_per_round": a.launches, "rounds": a.rounds,
           "timing": "one device-event pair around a graph replay of the back-to-back launches (no host launch rate), "
                     "one warm replay before each; contenders alternate per round",
           "kernels": kernels, "fast_rel_inf_vs_csr": fast_err,
           "speedup_exact_vs_csr": [min(us["csr"]) / max(us["exact"]), max(us["csr"]) / min(us["exact"])],
           "memory_bytes": {"F_D_G_tables_and_operator": mem_free, "assembled_A_with_row_blocks": mem_A}}

    if not a.no_solve:
        u, b = mp.manufactured_problem(n, xi=xi, etan=eta_n, etas=eta_s)
        bd = torch.from_numpy(b).cuda()
        nb = float(torch.linalg.vector_norm(bd))
        pc = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("mg", 6, accel="chebyshev"),
                                          inner_P=mp.InnerSolver("mg", 1), numerics="fast")
        for M in (op, A):                              # captures the apply's graph, warms every kernel of both runs
            mp.fgmres(M, bd, M=pc, tol=1e-8, maxiter=150)
        solves = {}
        for _ in range(a.rounds):                      # the two runs alternate: a solve is ~20 ms, one sample is noise
            for name, M in (("csr", A), ("exact", op)):
                hist = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                xs, info = mp.fgmres(M, bd, M=pc, tol=1e-8, maxiter=150, residuals=hist)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                s = solves.setdefault(name, {"seconds_rounds": []})
                s["seconds_rounds"].append(el)
                s.update({"iterations": len(hist) - 1, "converged": info == 0,
                          "true_rel_residual": float(torch.linalg.vector_norm(bd - A.matvec(xs))) / nb,
                          "velocity_max_error": float(np.max(np.abs(xs.cpu().numpy()[: 4 * N] - u[: 4 * N])))})
        for s in solves.values():
            s["seconds_min"], s["seconds_max"] = min(s["seconds_rounds"]), max(s["seconds_rounds"])
        assert len({s["iterations"] for s in solves.values()}) == 1, solves
        res["solve"] = {"preconditioner": "mg:6 accel=chebyshev / mg:1, fast numerics", "tol": 1e-8, "runs": solves}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
