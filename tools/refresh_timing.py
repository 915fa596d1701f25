"""Fresh construction against the in-place refresh of the approximate-Schur preconditioner (a time step: new thn field,
same grid), with a per-phase split of both, at eta_n = 100 and fast numerics.

    python tools/refresh_timing.py [--n 1024] [--out profiles/refresh_timing_1024.json]

Per configuration (chebyshev:4 / chebyshev:4; mg:1 / mg:1 at coarsest 16 and at coarsest 8):
  fresh    get_big_A_matrix + ApproxSchurPreconditioner(...) from scratch: the seconds of the SECOND build in the
           process (the first pays the cold start), and a third, instrumented build's seconds per phase
  refresh  refill + refresh on the same objects with a new field: the median of 5, each synchronised, one more with the
           per-phase split, and the peak extra device memory of one refresh
  galerkin per multigrid level, the fused values-only R (A P) launch (mpbp_triple_refill) against the two-spgemm build
           of the same level, device-event milliseconds

Phases: fill (operator values; fresh: count + scan + fill), products (Gt_G, Gt_F_G), galerkin (coarse operators),
diag_bounds (diagonals, Gershgorin bounds), host_pinv (coarsest level to the host, numpy pinv, back), layouts (SELL /
stencil-values copies; fresh: their plans and the row-block plans too), q13 (diamond values, symmetry check),
structure (fresh only: the transfers), other (the remainder of the synchronised total).
"""
import argparse
import contextlib
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import mp_block_preconditioners_amd as mpb
    from mp_block_preconditioners_amd import csr, mg, preconditioner, solve
    from mp_block_preconditioners_amd._lib import lib

    n = a.n
    dev = torch.device("cuda:0")
    depth = [0]

    @contextlib.contextmanager
    def phase(t, name):
        """csr.timed_phase, outermost block only (a SELL copy made inside a timed constructor counts once)."""
        if t is None or depth[0]:
            yield
            return
        depth[0] += 1
        try:
            with csr.timed_phase(t, name):
                yield
        finally:
            depth[0] -= 1

    @contextlib.contextmanager
    def instrumented(t):
        """The constructors' phases: the functions they call, wrapped for the duration of the block."""
        saved = []

        def wrap(owner, attr, name, kind="function"):
            fn = owner.__dict__[attr] if kind != "function" else getattr(owner, attr)
            raw = fn.__func__ if kind in ("classmethod", "staticmethod") else fn

            def timed(*args, **kw):
                with phase(t, name):
                    return raw(*args, **kw)
            saved.append((owner, attr, fn))
            setattr(owner, attr, {"classmethod": classmethod, "staticmethod": staticmethod}.get(kind, lambda f: f)(timed))
        wrap(mpb.MultiphaseBlockPreconditioner, "assemble", "fill", "method")
        wrap(preconditioner, "spgemm", "products")
        wrap(mg, "spgemm", "galerkin")
        wrap(mg, "transfer", "structure")
        wrap(mg, "dense_inverse_csr", "host_pinv")
        wrap(csr.DeviceCSR, "diagonal", "diag_bounds", "method")
        wrap(csr.DeviceCSR, "gershgorin", "diag_bounds", "method")
        wrap(csr.DeviceSELL, "from_csr", "layouts", "classmethod")
        wrap(csr.DeviceCSR, "plan_blocks", "layouts", "method")
        wrap(mg.StencilValues, "build", "layouts", "classmethod")
        wrap(solve, "_q13_layout", "q13")
        try:
            yield
        finally:
            for owner, attr, fn in reversed(saved):
                setattr(owner, attr, fn)

    def field(shift):
        """0.5 + 0.3 cos(2 pi (x + shift)) sin(4 pi y) at the three tables' points (device tensors)."""
        i = torch.arange(n * n, device=dev)
        r, c = (i // n).double(), (i % n).double()
        dx = 1.0 / n

        def f(y, x):
            return 0.5 + 0.3 * torch.cos(2 * torch.pi * (x + shift)) * torch.sin(4 * torch.pi * y)
        return f(-(r + 0.5) * dx, (c + 0.5) * dx), f(-(r + 0.5) * dx, c * dx), f(-r * dx, (c + 0.5) * dx)

    def build(inner, coarsest):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bp = mpb.MultiphaseBlockPreconditioner(n, 1.0, 100.0, 1.0, device=dev)
        ops = bp.get_big_A_matrix(c=1.0, d_u=-1.0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        kind, _, k = inner.partition(":")
        kw = dict(coarsest=coarsest) if coarsest else {}
        pc = mpb.ApproxSchurPreconditioner(ops[2], ops[3], ops[4], inner_F=mpb.InnerSolver(kind, int(k), **kw),
                                           inner_P=mpb.InnerSolver(kind, int(k), **kw), numerics="fast")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return bp, ops, pc, {"assemble_s": t1 - t0, "constructor_s": t2 - t1, "total_s": t2 - t0}

    def step(bp, ops, pc, tabs, t=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bp.update_theta_tables(*tabs)
        with phase(t, "fill"):
            bp.refill(ops[0], ops[2], ops[3], ops[4], c=1.0, d_u=-1.0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pc.refresh(timings=t)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return {"refill_s": t1 - t0, "refresh_s": t2 - t1, "total_s": t2 - t0}

    def rounded(d):
        return {k: round(v, 5) for k, v in d.items()}

    def with_other(t, total):
        t = dict(t)
        t["other"] = total - sum(t.values())
        return rounded(t)

    def galerkin_levels(pc):
        """Per level >= 1 of both hierarchies: the fused refill's and the two-spgemm build's device-event ms."""
        import ctypes

        from mp_block_preconditioners_amd import _lib
        out = []
        for name, h in (("F", pc.mg_F), ("Gt_G", pc.mg_P)):
            if h is None:
                continue
            for l in range(1, h.nlevels):
                R, A, P, C = h.R[l - 1], h.ops[l - 1], h.P[l - 1], h.ops[l]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record()
                _lib.check(lib().mpbp_triple_refill(ctypes.byref(R.cstruct()), ctypes.byref(A.cstruct()),
                                                    ctypes.byref(P.cstruct()), _lib.ASSOC_RIGHT, 1.0, 1.0,
                                                    ctypes.byref(C.cstruct()), _lib.stream_handle()))
                ev[1].record()
                ev[2].record()
                ref = csr.spgemm(R, csr.spgemm(A, P))
                ev[3].record()
                torch.cuda.synchronize()
                out.append({"hierarchy": name, "level": l, "rows": C.shape[0], "nnz": C.nnz,
                            "fused_refill_ms": round(ev[0].elapsed_time(ev[1]), 4),
                            "two_spgemm_build_ms": round(ev[2].elapsed_time(ev[3]), 4),
                            "same_bits": bool(torch.equal(ref.val, C.val))})
                del ref
        return out

    res = {"n": n, "eta_n": 100.0, "numerics": "fast", "device": torch.cuda.get_device_name(0), "configs": []}
    for inner, coarsest in (("chebyshev:4", None), ("mg:1", 16), ("mg:1", 8)):
        builds = []
        for i in range(3):
            t = {} if i == 2 else None
            with (instrumented(t) if t is not None else contextlib.nullcontext()):
                bp, ops, pc, secs = build(inner, coarsest)
            builds.append(secs)
            if i < 2:
                del bp, ops, pc
                torch.cuda.empty_cache()
        fresh_phases = with_other(t, builds[2]["total_s"])
        tabs = [field(0.05 * (i + 1)) for i in range(7)]
        torch.cuda.synchronize()
        runs = [step(bp, ops, pc, tabs[i]) for i in range(5)]
        t = {}
        timed = step(bp, ops, pc, tabs[5], t)
        refresh_phases = with_other(t, timed["total_s"])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(bp, ops, pc, tabs[6])
        peak = torch.cuda.max_memory_allocated() - base
        v = torch.ones(pc.shape[0], dtype=torch.float64, device=dev)
        out = torch.empty_like(v)
        g = pc.capture(v, out)      # capture() after refresh() works
        g.replay()
        torch.cuda.synchronize()
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        cfg = {"inner_F": inner, "inner_P": inner, "coarsest": coarsest,
               "fresh_second_build": rounded(builds[1]), "fresh_first_build_cold": rounded(builds[0]),
               "fresh_phases_instrumented_build": fresh_phases,
               "refresh_median_of_5": rounded(med), "refresh_runs_total_s": [round(r["total_s"], 5) for r in runs],
               "refresh_phases_instrumented_run": refresh_phases,
               "refresh_peak_extra_device_bytes": int(peak), "kept_device_bytes": int(base),
               "speedup_total": round(builds[1]["total_s"] / med["total_s"], 2),
               "speedup_constructor_vs_refresh": round(builds[1]["constructor_s"] / med["refresh_s"], 2),
               "galerkin_levels": galerkin_levels(pc), "generation": pc.generation}
        res["configs"].append(cfg)
        print(json.dumps(cfg), flush=True)
        del bp, ops, pc, g, tabs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
