"""Multigrid on any grid size (InnerSolver("mg", ..., coarsen="any")) next to the default rule, fast numerics.

    python tools/mg_any_timing.py [--rounds 5] [--out profiles/mg_any_1000.json]

n = 1000 with coarsen="any" (1000, 500, 250, 125, 62, 31, 15) against n = 1024 under the default rule, in the same
process and in alternating rounds (min - max over the rounds):
  apply    the mg:1 / mg:1 Schur apply, hipGraph replay, milliseconds
  build    get_big_A_matrix's operators given, ApproxSchurPreconditioner(...) seconds; refresh: refill + refresh seconds
  fgmres   iterations and seconds to tol 1e-8 at eta_n = 100 and eta ratio 1e4, for mg:1 / mg:1 and for
           InnerSolver("mg", 6, accel="chebyshev") / mg:1
and n = 100: build and refresh with coarsen="any" (100, 50, 25, 12) against the default rule's three levels with a
2500-row dense coarsest level.  Also records which levels hold a stencil-values copy (levels 0-2 of n = 1000 are even
sizes and take the kernels they take under the default rule)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import mp_block_preconditioners_amd as mpb

    def sync():
        torch.cuda.synchronize()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return r, time.perf_counter() - t0

    def system(n, eta_n):
        bp = mpb.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
        A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
        return bp, (A, F, D, G)

    def inner(coarsen, cycles=1, **kw):
        return mpb.InnerSolver("mg", cycles, coarsen=coarsen, **kw)

    def apply_ms(pc, reps=50):
        v = torch.from_numpy(np.random.default_rng(0).standard_normal(pc.shape[0])).cuda()
        out = torch.empty_like(v)
        g = pc.capture(v, out)
        for _ in range(5):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    def solve(A, pc, n, eta_n):
        _, b = mpb.manufactured_problem(n, etan=eta_n, etas=1.0)
        bd = torch.from_numpy(b).cuda()
        hist = []
        (_, info), secs = timed(lambda: mpb.fgmres(A, bd, M=pc, tol=1e-8, maxiter=150, residuals=hist))
        return dict(iterations=len(hist) - 1, info=int(info), seconds=secs)

    def one_round(n, coarsen, eta_n, full):
        bp, (A, F, D, G) = system(n, eta_n)
        pc, build = timed(lambda: mpb.ApproxSchurPreconditioner(F, D, G, inner_F=inner(coarsen), inner_P=inner(coarsen),
                                                                numerics="fast"))
        rec = dict(build_s=build, levels=pc.mg_F.sizes, svl_levels=[V is not None for V in pc.mg_F.svls])
        if full:
            rec["apply_ms"] = apply_ms(pc)
            rec["fgmres_mg1_mg1"] = solve(A, pc, n, eta_n)
            pc6 = mpb.ApproxSchurPreconditioner(F, D, G, inner_F=inner(coarsen, 6, accel="chebyshev"),
                                                inner_P=inner(coarsen), numerics="fast")
            rec["fgmres_cheb6_mg1"] = solve(A, pc6, n, eta_n)
            rec["rho_F"] = pc6.mg_F.rho
            del pc6
        # a time step: a new (smooth) volume-fraction field on the same grid, refill + refresh in place
        i = torch.arange(n * n, device="cuda")
        r, c = (i // n).double(), (i % n).double()
        dx = 1.0 / n

        def f(y, x):
            return 0.5 + 0.3 * torch.cos(2 * torch.pi * x) * torch.sin(4 * torch.pi * y)
        tabs = (f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx))

        def step():
            bp.update_theta_tables(*tabs)
            bp.refill(A, F, D, G, c=1.0, d_u=-1.0)
            pc.refresh()
        _, rec["refresh_s"] = timed(step)
        return rec

    cases = [("n1000_any", 1000, "any", True), ("n1024_even", 1024, "even", True),
             ("n100_any", 100, "any", False), ("n100_even", 100, "even", False)]
    one_round(64, "even", 100.0, True)   # cold start
    runs = {}
    for eta_n in (100.0, 1.0e4):
        for r in range(a.rounds):
            for name, n, coarsen, full in cases:
                if not full and eta_n != 100.0:
                    continue
                rec = one_round(n, coarsen, eta_n, full)
                runs.setdefault(f"{name}_eta{eta_n:g}", []).append(rec)
                print(f"eta_n={eta_n:g} round {r} {name}: {json.dumps(rec)}", flush=True)
                torch.cuda.empty_cache()

    def span(recs, *path):
        vals = []
        for rec in recs:
            v = rec
            for k in path:
                v = v[k]
            vals.append(v)
        return [min(vals), max(vals)]

    summary = {}
    for key, recs in runs.items():
        s = dict(levels=recs[0]["levels"], svl_levels=recs[0]["svl_levels"], build_s=span(recs, "build_s"),
                 refresh_s=span(recs, "refresh_s"))
        if "apply_ms" in recs[0]:
            s["apply_ms"] = span(recs, "apply_ms")
            for cfg in ("fgmres_mg1_mg1", "fgmres_cheb6_mg1"):
                s[cfg] = dict(iterations=span(recs, cfg, "iterations"), seconds=span(recs, cfg, "seconds"),
                              info=span(recs, cfg, "info"))
        summary[key] = s
    doc = dict(what="coarsen='any' at n = 1000 against the default rule at n = 1024 (fast numerics, alternating rounds, "
                    "[min, max]); n = 100 build / refresh under both rules",
               device=torch.cuda.get_device_name(0), rounds=a.rounds, summary=summary, runs=runs)
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
