"""Chebyshev-accelerated against stationary F V-cycles at the solve level: FGMRES (tol 1e-8, x0 = 0) on the reference's
manufactured problem (solve.py:52-80) at 1024^2, fast numerics, inner_P = mg:1, with inner_F = mg:4, mg:8 and the
accelerated K = 3, 4, 5, 6 (rho estimated).  Every case is built and warmed first (its apply captured, one solve run);
the timed rounds then alternate the variants inside this one process.

    python tools/mg_accel_study.py [--n 1024] [--eta-n 100 1e4] [--rounds 5] [--out profiles/mg_accel_study_1024.jsonl]

One JSON line per (eta_n, variant): iterations, apply ms (graph replay, device events), solve seconds (median and every
round), the estimated rho and the seconds one estimate takes; and one line per eta_n for k_mg_combine (mpbp_mg_combine,
the k >= 2 form with sub: four reads and one write of level 0's length, 168 MB at 1024^2) beside mpbp_hbm_stream
moving the same number of bytes (mode 0: read once; mode 1: the SpMV's read-mostly stream shape), device-event ms.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("mg:4", 4, None), ("mg:8", 8, None), ("accel:3", 3, "chebyshev"), ("accel:4", 4, "chebyshev"),
            ("accel:5", 5, "chebyshev"), ("accel:6", 6, "chebyshev")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--eta-n", type=float, nargs="+", default=[100.0, 1e4])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="graph replays per apply timing")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd._lib import check, lib, ptr, stream_handle
    from mp_block_preconditioners_amd.solve import DeviceEvent

    n = a.n
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def event_ms(fn, reps):
        e0, e1 = DeviceEvent(), DeviceEvent()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / reps

    for eta_n in a.eta_n:
        bp = mp.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
        A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
        u, b = mp.manufactured_problem(n, xi=1.0, etan=eta_n, etas=1.0)
        bd = torch.from_numpy(b).cuda()
        nb = float(torch.linalg.vector_norm(bd))
        cases = []
        for name, K, accel in VARIANTS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M = mp.ApproxSchurPreconditioner(F, D, G, inner_F=mp.InnerSolver("mg", K, accel=accel),
                                             inner_P=mp.InnerSolver("mg", 1), numerics="fast")
            torch.cuda.synchronize()
            c = {"name": name, "K": K, "accel": accel, "M": M, "setup_s": time.perf_counter() - t0, "rho": M.mg_F.rho,
                 "rho_estimate_s": None, "apply_ms": [], "solve_s": []}
            if accel:   # one more estimate, timed on its own (the constructor's is inside setup_s)
                t0 = time.perf_counter()
                again = M.mg_F.estimate_rho()
                torch.cuda.synchronize()
                c["rho_estimate_s"] = time.perf_counter() - t0
                c["rho_repeatable"] = again == M.mg_F.rho
                c["contraction_ratios"] = M.mg_F.contraction()
            v = torch.randn(M.shape[0], dtype=torch.float64, device="cuda",
                            generator=torch.Generator(device="cuda").manual_seed(1))
            out = torch.empty_like(v)
            c["graph"], c["v"], c["out"] = M.capture(v, out), v, out
            c["graph"].replay()
            hist = []
            x, info = mp.fgmres(A, bd, M=M, tol=a.tol, maxiter=a.maxiter, residuals=hist)   # warm: fgmres captures M once
            torch.cuda.synchronize()
            c["iterations"], c["converged"] = len(hist) - 1, info == 0
            c["true_rel_residual"] = float(torch.linalg.vector_norm(bd - A.matvec(x))) / nb
            c["residuals"] = [float(r) for r in hist]
            del x
            cases.append(c)
        for _ in range(a.rounds):   # alternate the variants
            for c in cases:
                c["apply_ms"].append(event_ms(c["graph"].replay, a.reps))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x, info = mp.fgmres(A, bd, M=c["M"], tol=a.tol, maxiter=a.maxiter)
                torch.cuda.synchronize()
                c["solve_s"].append(time.perf_counter() - t0)
                del x
        for c in cases:
            emit({"n": n, "eta_n": eta_n, "numerics": "fast", "inner_F": c["name"], "inner_P": "mg:1", "cycles": c["K"],
                  "accel": c["accel"], "rho": c["rho"], "rho_estimate_s": c["rho_estimate_s"],
                  "rho_repeatable": c.get("rho_repeatable"), "contraction_ratios": c.get("contraction_ratios"),
                  "iterations": c["iterations"], "converged": c["converged"], "true_rel_residual": c["true_rel_residual"],
                  "apply_ms": statistics.median(c["apply_ms"]), "apply_ms_rounds": c["apply_ms"],
                  "solve_s": statistics.median(c["solve_s"]), "solve_s_rounds": c["solve_s"], "setup_s": c["setup_s"],
                  "residuals": c["residuals"], "device": torch.cuda.get_device_name(0)})
        # the combination kernel beside the HBM calibration streams of the same byte count, alternating
        n0 = F.shape[0]
        vec = [torch.randn(n0, dtype=torch.float64, device="cuda") for _ in range(5)]
        nbytes = 5 * 8 * n0
        src = torch.randn(nbytes // 8, dtype=torch.float64, device="cuda")
        sink = torch.zeros(max(256, nbytes // 144 + 64), dtype=torch.float64, device="cuda")

        def combine():
            check(lib().mpbp_mg_combine(n0, ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), 1.05, 7e-4, ptr(vec[3]), ptr(vec[4]),
                                        stream_handle()))

        def stream(mode):
            return lambda: check(lib().mpbp_hbm_stream(ptr(src), nbytes, mode, ptr(sink), stream_handle()))
        kinds = {"k_mg_combine": combine, "hbm_stream_read": stream(0), "hbm_stream_readwrite": stream(1)}
        for fn in kinds.values():
            event_ms(fn, 3)
        ms = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for k, fn in kinds.items():
                ms[k].append(event_ms(fn, 20))
        rec = {"n": n, "eta_n": eta_n, "kernel": "k_mg_combine", "elements": n0, "bytes": nbytes}
        for k in kinds:
            med = statistics.median(ms[k])
            rec[k + "_ms"] = med
            rec[k + "_GBps"] = nbytes / med / 1e6
            rec[k + "_ms_rounds"] = ms[k]
        emit(rec)
        del cases, vec, src, sink, A, F, D, G, bp
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
