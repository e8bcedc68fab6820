#!/usr/bin/env python3
"""What a term objective compiled at run time costs, in one process on one device (profiles/term_objective.json).

  single  extended Rosenbrock, n = 1e8 f64, m = 10, More-Thuente: time of a whole minimise (device events around it; the
          wall clock beside them) divided by its evaluations for
          (a) the built-in ExtendedRosenbrock, (b) the same objective as a TermObjective, (c) the same objective as a torch
          DeviceObjective.  One warm-up round, then the legs alternate; x lives on the device, so a minimise moves no host data.
  box     cfg4's shape (box QP, n = 1e7 f64, m = 10, bounds +-1): the built-in DiagQuadratic against the TermObjective with a, b
          as device arrays; per minimise the iterations per second and how many first trials rode on the dg / max-step pass.
  compile the one-off hipRTC time of each body (as lbfgsx_objective_info reports it).
The single-problem L-BFGS path has no speculative first trial inside its persistent launch, so every evaluation of (a) and (b)
is the same launch of the same kernel text: `evaluations_through_speculative_trial` is reported and is 0.

    python scripts/measure_term_objective.py [--out profiles/term_objective.json] [--single-n 100000000] [--box-n 10000000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROSEN = """const T t1 = T(1) - x[0];
const T t2 = T(10) * (x[1] - x[0] * x[0]);
g[1] = T(20) * t2;
g[0] = T(-2) * (x[0] * g[1] + t1);
return t1 * t1 + t2 * t2;"""
QUAD = """const T r = p0[i] * x[0] - p1[i];
g[0] = p0[i] * r;
return T(0.5) * (r * r);"""


def rosen_single(torch):
    def fn(x, g):
        x0, x1 = x[0::2], x[1::2]
        t1 = 1.0 - x0
        t2 = 10.0 * (x1 - x0 * x0)
        g1 = 20.0 * t2
        g[1::2] = g1
        g[0::2] = -2.0 * (x0 * g1 + t1)
        return float((t1 * t1 + t2 * t2).sum())
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "term_objective.json"))
    ap.add_argument("--single-n", type=int, default=100000000)
    ap.add_argument("--box-n", type=int, default=10000000)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--box-iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_term_objective.py needs a GPU")
    rec = {"device": torch.cuda.get_device_name(0)}
    term_rosen, term_quad = A.TermObjective(ROSEN, K=2), A.TermObjective(QUAD)
    rec["compile"] = {"rosenbrock_f64": term_rosen.info(), "quadratic_f64": term_quad.info()}

    n1 = args.single_n
    single = {"n": n1, "dtype": "f64", "m": 10, "iterations": args.iters, "built_in": [], "term_objective": [], "torch_callback": [],
              "evaluations_through_speculative_trial": 0}
    s = A.LBFGSSolver(A.LBFGSParam(m=10, epsilon=0.0, epsilon_rel=0.0, max_iterations=args.iters), linesearch=A.LS_MORE_THUENTE)
    xd = torch.empty(n1, dtype=torch.float64, device="cuda:0")
    start = torch.where(torch.arange(n1, device="cuda:0") % 2 == 1, 1.0, -1.2).double()
    legs = (("built_in", A.ExtendedRosenbrock()), ("term_objective", term_rosen), ("torch_callback", A.DeviceObjective(rosen_single(torch))))
    for rnd in range(args.rounds):  # round 0 warms every leg up
        for name, f in legs:
            xd.copy_(start)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            niter, fx = s.minimize(f, xd)
            dt = time.perf_counter() - t0
            e1.record()
            e1.synchronize()
            if rnd:
                single[name].append({"s": dt, "event_ms": e0.elapsed_time(e1), "niter": niter, "nfev": s.last.nfev, "fx": fx,
                                     "ms_per_evaluation_of_the_whole_solve": e0.elapsed_time(e1) / s.last.nfev})
    med = {k: float(np.median([r["ms_per_evaluation_of_the_whole_solve"] for r in single[k]])) for k, _ in legs}
    single["median_ms_per_evaluation"] = med
    single["term_over_built_in"] = med["term_objective"] / med["built_in"]
    single["torch_over_term"] = med["torch_callback"] / med["term_objective"]
    rec["single"] = single
    s.close()
    del xd, start
    torch.cuda.empty_cache()

    nb = args.box_n
    rng = np.random.default_rng(1)
    a = torch.as_tensor(1.0 + 9.0 * rng.random(nb), device="cuda:0")
    b = torch.as_tensor(rng.standard_normal(nb) * 5.0, device="cuda:0")
    term_quad.set_data(a, b)
    box = {"n": nb, "dtype": "f64", "m": 10, "iterations": args.box_iters, "built_in": [], "term_objective": []}
    sb = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=0.0, epsilon_rel=0.0, past=0, max_iterations=args.box_iters))
    from lbfgspp_amd import _lib as L
    ctx = sb.prepare(nb)  # the built-in quadratic reads its a, b from the context's own vectors: placed there once
    for which, src in ((L.VEC_A, a), (L.VEC_B, b)):
        L.device_tensor(core.lbfgsx_vec(ctx, which), (nb,), np.float64, 0).copy_(src)
    torch.cuda.synchronize()
    lb, ub = -torch.ones(nb, dtype=torch.float64, device="cuda:0"), torch.ones(nb, dtype=torch.float64, device="cuda:0")
    xb = torch.zeros(nb, dtype=torch.float64, device="cuda:0")
    for rnd in range(args.rounds):
        for name, f in (("built_in", A.DiagQuadratic()), ("term_objective", term_quad)):
            xb.zero_()
            torch.cuda.synchronize()
            ahead0 = (C.c_int64 * 2)()
            core.lbfgsx_b_trial_ahead_counts(sb.ctx, C.byref(ahead0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            niter, fx = sb.minimize(f, xb, lb, ub)
            dt = time.perf_counter() - t0
            e1.record()
            e1.synchronize()
            ahead = (C.c_int64 * 2)()
            core.lbfgsx_b_trial_ahead_counts(sb.ctx, C.byref(ahead))
            if rnd:
                box[name].append({"s": dt, "event_ms": e0.elapsed_time(e1), "niter": niter, "nfev": sb.last.nfev, "fx": fx, "iterations_per_s": niter / dt,
                                  "first_trials_ahead": ahead[0] - ahead0[0], "taken_over": ahead[1] - ahead0[1]})
    box["term_over_built_in_time"] = float(np.median([r["s"] for r in box["term_objective"]]) / np.median([r["s"] for r in box["built_in"]]))
    rec["box"] = box
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"single": single["median_ms_per_evaluation"], "term_over_built_in": single["term_over_built_in"],
                      "torch_over_term": single["torch_over_term"], "box_term_over_built_in_time": box["term_over_built_in_time"]}))


if __name__ == "__main__":
    main()
