"""The four block forms of the Schur preconditioner (ApproxSchurPreconditioner(form=...)) at the apply and at the solve
level: one process, 1024^2, fast numerics, hipGraph applies, FGMRES (tol 1e-8, x0 = 0, maxiter 150) on the reference's
manufactured problem (solve.py:52-80) at eta_n = 100 and eta_n = 1e4.

    python tools/block_forms_study.py [--n 1024] [--eta-n 100 1e4] [--rounds 5] [--out profiles/block_forms_1024.json]

Inner configurations (inner_F / inner_P): chebyshev:4 / chebyshev:4 (apply only: four sweeps do not make a solver),
mg:1 / mg:1, mg:4 / mg:1, mg:8 / mg:1 and InnerSolver("mg", 6, accel="chebyshev") / mg:1.  Per configuration the forms
are built and warmed first (apply captured, one solve run), then the timed rounds alternate the forms, so a drift of the
machine falls on all of them alike; every figure is reported as median and min-max over the rounds.  For the upper form
with chebyshev:4 the right-hand side v_u - G x_p built inside the F solve launch (fuse_g) is timed against the G launch +
solve pair in the same rounds.  Apply ms: device events around `reps` graph replays; solve seconds: a host clock around
fgmres ending in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("full", "upper", "lower", "diagonal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--eta-n", type=float, nargs="+", default=[100.0, 1e4])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="graph replays per apply timing")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import mp_block_preconditioners_amd as mp
    from mp_block_preconditioners_amd.solve import DeviceEvent

    assert torch.cuda.is_available(), "block_forms_study needs a GPU"
    n = a.n
    IS = mp.InnerSolver
    configs = [("chebyshev:4/chebyshev:4", lambda: IS("chebyshev", 4), lambda: IS("chebyshev", 4), False),
               ("mg:1/mg:1", lambda: IS("mg", 1), lambda: IS("mg", 1), True),
               ("mg:4/mg:1", lambda: IS("mg", 4), lambda: IS("mg", 1), True),
               ("mg:8/mg:1", lambda: IS("mg", 8), lambda: IS("mg", 1), True),
               ("accel:6/mg:1", lambda: IS("mg", 6, accel="chebyshev"), lambda: IS("mg", 1), True)]
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

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

    for eta_n in a.eta_n:
        bp = mp.MultiphaseBlockPreconditioner(n, 1.0, eta_n, 1.0)
        A, _, F, D, G = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
        _, b = mp.manufactured_problem(n, xi=1.0, etan=eta_n, etas=1.0)
        bd = torch.from_numpy(b).cuda()
        nb = float(torch.linalg.vector_norm(bd))
        products = ()
        for name, mk_f, mk_p, solves in configs:
            variants = [(form, True) for form in FORMS]
            if not solves:
                variants.append(("upper", False))   # the G launch + solve pair beside the fused right-hand side
            cases = []
            for form, fuse_g in variants:
                M = mp.ApproxSchurPreconditioner(F, D, G, *products, inner_F=mk_f(), inner_P=mk_p(), numerics="fast",
                                                 form=form, fuse_g=fuse_g)
                products = (M.GtG, M.GtFG)
                c = {"form": form, "M": M, "fuse_g": M.fuse_g, "apply_ms": [], "solve_s": []}
                v = torch.randn(M.shape[0], dtype=torch.float64, device="cuda",
                                generator=torch.Generator(device="cuda").manual_seed(1))
                out = torch.empty_like(v)
                c["graph"], c["v"], c["out"] = M.capture(v, out), v, out
                c["graph"].replay()
                if solves:   # warm: fgmres captures M once
                    hist = []
                    x, info = mp.fgmres(A, bd, M=M, tol=a.tol, maxiter=a.maxiter, residuals=hist)
                    torch.cuda.synchronize()
                    c["iterations"], c["converged"] = len(hist) - 1, info == 0
                    c["true_rel_residual"] = float(torch.linalg.vector_norm(bd - A.matvec(x))) / nb
                    del x
                torch.cuda.synchronize()
                cases.append(c)
            if not solves:   # the fused right-hand side changes no bit
                fused, apart = cases[1], cases[-1]
                assert fused["fuse_g"] and not apart["fuse_g"] and torch.equal(fused["out"], apart["out"])
            for _ in range(a.rounds):   # alternate the forms
                for c in cases:
                    c["apply_ms"].append(event_ms(c["graph"].replay, a.reps))
                    if solves:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        x, info = mp.fgmres(A, bd, M=c["M"], tol=a.tol, maxiter=a.maxiter)
                        torch.cuda.synchronize()
                        c["solve_s"].append(time.perf_counter() - t0)
                        del x
            for c in cases:
                rec = {"n": n, "eta_n": eta_n, "numerics": "fast", "inner": name, "form": c["form"],
                       "fuse_g": c["fuse_g"], "apply_ms": spread(c["apply_ms"])}
                if solves:
                    rec.update(iterations=c["iterations"], converged=c["converged"],
                               true_rel_residual=c["true_rel_residual"], solve_s=spread(c["solve_s"]))
                emit(rec)
            del cases
            torch.cuda.empty_cache()
        del A, F, D, G, bp, products
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "n": n, "rounds": a.rounds, "reps": a.reps,
                       "tol": a.tol, "maxiter": a.maxiter, "records": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
