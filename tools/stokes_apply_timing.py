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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eta-n", type=float, default=100.0)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 1 or a.rounds < 1:
        ap.error("--launches and --rounds must be positive")
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
