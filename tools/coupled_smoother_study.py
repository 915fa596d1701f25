"""The phase-coupled multigrid smoother (InnerSolver("mg", k, smoother="coupled")) against the point smoother over the
drag xi: one process, 1024^2, fast numerics, hipGraph applies, FGMRES (tol 1e-8, x0 = 0, maxiter 150) on the reference's
manufactured problem (solve.py:52-80).

    python tools/coupled_smoother_study.py [--n 1024] [--xi 1 1e4 1e6 1e8] [--eta 100/1 1/1] [--rounds 5]
                                           [--out profiles/coupled_smoother_1024.json]

Per (eta_n / eta_s, xi): inner_F mg:1 and the Chebyshev-accelerated mg:6 (rho estimated; a cycle that does not contract
is refused there and recorded as such), inner_P mg:1, each with smoother "point" and "coupled".  Everything of one
(eta, xi) is built and warmed first (apply captured, one solve run), then the timed rounds alternate the cases, so a
drift of the machine falls on all of them alike; figures are median and min-max over the rounds.  The coupled cases
are timed a second time with the level-0 sweep as two launches (Multigrid.set_coupled_fuse(False)) in the same rounds.
Apply ms: device events around `reps` graph replays; solve seconds: a host clock around fgmres ending in a device
synchronise; contraction: Multigrid.contraction(steps) of the F hierarchy, last ratio."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--xi", type=float, nargs="+", default=[1.0, 1e4, 1e6, 1e8])
    ap.add_argument("--eta", nargs="+", default=["100/1", "1/1"], help="eta_n/eta_s pairs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="graph replays per apply timing")
    ap.add_argument("--steps", type=int, default=8, help="power steps of the contraction estimate")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", default=None, help="append each record as a JSON line as soon as it is measured")
    a = ap.parse_args()
    import torch

    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd.solve import DeviceEvent

    assert torch.cuda.is_available(), "coupled_smoother_study needs a GPU"
    n = a.n
    IS = mp.InnerSolver
    inners = [("mg:1/mg:1", lambda s: IS("mg", 1, smoother=s)),
              ("accel:6/mg:1", lambda s: IS("mg", 6, accel="chebyshev", smoother=s))]
    records = []

    def emit(rec):
        records.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.log:
            with open(a.log, "a") as f:
                f.write(line + "\n")

    def event_ms(fn, reps):
        e0, e1 = DeviceEvent(), DeviceEvent()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / reps

    def spread(xs):
        return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": xs}

    for eta in a.eta:
        eta_n, eta_s = (float(t) for t in eta.split("/"))
        for xi in a.xi:
            bp = mp.MultiphaseBlockPreconditioner(n, xi, eta_n, eta_s)
            A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
            _, b = mp.manufactured_problem(n, xi=xi, etan=eta_n, etas=eta_s)
            bd = torch.from_numpy(b).cuda()
            nb = float(torch.linalg.vector_norm(bd))
            products, cases = (), []
            for name, mk_f in inners:
                for smoother in ("point", "coupled"):
                    base = {"n": n, "xi": xi, "eta_n": eta_n, "eta_s": eta_s, "numerics": "fast", "inner": name,
                            "smoother": smoother}
                    try:
                        M = mp.ApproxSchurPreconditioner(F, D, G, *products, inner_F=mk_f(smoother), inner_P=IS("mg", 1),
                                                         numerics="fast")
                    except ValueError as e:   # accel: the estimated rho is not below ACCEL_RHO_MAX
                        emit({**base, "refused": str(e)[:160]})
                        continue
                    products = (M.GtG, M.GtFG)
                    v = torch.randn(M.shape[0], dtype=torch.float64, device="cuda",
                                    generator=torch.Generator(device="cuda").manual_seed(1))
                    forms = [("fused" if smoother == "coupled" else None, True)]
                    if smoother == "coupled":
                        forms.append(("two-launch", False))
                    for label, fuse in forms:
                        M.mg_F.set_coupled_fuse(fuse)
                        out = torch.empty_like(v)
                        c = {**base, "level0": label, "M": M, "fuse": fuse, "v": v, "out": out,
                             "graph": M.capture(v, out), "apply_ms": [], "solve_s": []}
                        c["graph"].replay()
                        torch.cuda.synchronize()
                        cases.append(c)
                    M.mg_F.set_coupled_fuse(True)
                    c = cases[-len(forms)]
                    c["contraction"] = M.mg_F.contraction(steps=a.steps)[-1]
                    c["rho"] = M.mg_F.rho
                    hist = []
                    x, info = mp.fgmres(A, bd, M=M, tol=a.tol, maxiter=a.maxiter, residuals=hist)   # (warm)
                    torch.cuda.synchronize()
                    c["iterations"], c["converged"] = len(hist) - 1, info == 0
                    c["true_rel_residual"] = float(torch.linalg.vector_norm(bd - A.matvec(x))) / nb
                    del x
            for c in cases:   # the two level-0 forms of a coupled case apply the same operator
                if c["level0"] == "two-launch":
                    fused = next(k for k in cases if k["M"] is c["M"] and k["level0"] == "fused")
                    c["max_abs_diff_to_fused"] = float((c["out"] - fused["out"]).abs().max())
            for _ in range(a.rounds):   # alternate the cases
                for c in cases:
                    c["apply_ms"].append(event_ms(c["graph"].replay, a.reps))
                    if "iterations" in c:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        x, info = mp.fgmres(A, bd, M=c["M"], tol=a.tol, maxiter=a.maxiter)
                        torch.cuda.synchronize()
                        c["solve_s"].append(time.perf_counter() - t0)
                        del x
            for c in cases:
                rec = {k: v for k, v in c.items() if k not in ("M", "v", "out", "graph", "fuse", "apply_ms", "solve_s")}
                rec["apply_ms"] = spread(c["apply_ms"])
                if c["solve_s"]:
                    rec["solve_s"] = spread(c["solve_s"])
                emit(rec)
            del cases, products, A, F, D, G, bp
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "n": n, "rounds": a.rounds, "reps": a.reps,
                       "steps": a.steps, "tol": a.tol, "maxiter": a.maxiter, "records": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
