#!/usr/bin/env python3
"""What a chain objective (overlapping terms, lbfgspp_amd.ChainObjective) costs, in one process on one device
(profiles/chain_objective.json).

  trial   n = 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of the timed calls after warm-up, the tile order alternating as in a search) for
          (a) the built-in ExtendedRosenbrock, (b) the K = 2 chained Rosenbrock, (c) the K = 3 second difference -- without
          data arrays (the four streams of (a)) and as the weighted fit with two data arrays (six streams) -- and (d) the torch
          callable of (b) (trial point + callable + grad.d, what a DeviceObjective costs per evaluation).
          The yardstick of (b) and (c) is (a) of the same run: the bytes are the same.
  box     cfg4's shape (n = 1e7 f64, m = 10) under L-BFGS-B: the chained Rosenbrock in the box [-0.5, 2] beside the built-in
          quadratic in [-1, 1]; iterations per second and how many first trials rode on the dg / max-step pass.
  code    VGPRs and scratch of each compiled body, from the code object.

    python scripts/measure_chain_objective.py [--out profiles/chain_objective.json] [--n 100000000] [--box-n 10000000]
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

CHAINED_ROSEN = """const T u = x[1] - x[0] * x[0];
const T v = T(1) - x[0];
g[1] = T(200) * u;
g[0] = T(-400) * (u * x[0]) - T(2) * v;
return T(100) * (u * u) + v * v;"""
SECOND_DIFF = """const T s = (x[0] - T(2) * x[1]) + x[2];
const T w = T(2) * (c[0] * s);
g[0] = w + c[1] * x[0];
g[1] = T(-2) * w;
g[2] = w;
return c[0] * (s * s) + (T(0.5) * c[1]) * (x[0] * x[0]);"""
SECOND_DIFF_FIT = """const T r = x[0] - p1[i];
const T s = (x[0] - T(2) * x[1]) + x[2];
const T w = T(2) * (c[0] * s);
g[0] = T(2) * (p0[i] * r) + w;
g[1] = T(-2) * w;
g[2] = w;
return p0[i] * (r * r) + c[0] * (s * s);"""


def chained_rosen_torch(torch):
    def fn(x, g):
        x0, x1 = x[:-1], x[1:]
        u = x1 - x0 * x0
        v = 1.0 - x0
        g.zero_()
        g[1:] += 200.0 * u
        g[:-1] += -400.0 * (u * x0) - 2.0 * v
        return float((100.0 * (u * u) + v * v).sum())
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_objective.json"))
    ap.add_argument("--n", type=int, default=100000000)
    ap.add_argument("--box-n", type=int, default=10000000)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--box-iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_chain_objective.py needs a GPU")
    rec = {"device": torch.cuda.get_device_name(0)}
    bodies = {"chained_rosenbrock": A.ChainObjective(CHAINED_ROSEN, K=2), "second_difference": A.ChainObjective(SECOND_DIFF, K=3),
              "second_difference_fit": A.ChainObjective(SECOND_DIFF_FIT, K=3)}
    rec["code"] = {k: f.info() for k, f in bodies.items()}

    # ---- one trial evaluation at n
    n = args.n
    h = C.c_void_p()
    L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))

    def vec(which):
        return L.device_tensor(core.lbfgsx_vec(h, which), (n,), np.float64, 0)

    gen = torch.Generator(device="cuda:0").manual_seed(1)
    vec(L.VEC_X).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
    vec(L.VEC_D).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
    p0 = 1.0 + torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen)
    p1 = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen)
    torch.cuda.synchronize()
    L.check(core.lbfgsx_ls_begin(h))
    fx, dg = C.c_double(), C.c_double()

    def bind(f, data=(), scalars=()):
        ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in data])
        cs = (C.c_double * 8)(*(tuple(scalars) + (0.0,) * (8 - len(scalars))))
        oid = C.c_int(-1)
        L.check(core.lbfgsx_objective_bind(h, f.compile(), C.byref(ptrs), C.byref(cs), C.byref(oid)))
        return oid.value

    fn = chained_rosen_torch(torch)

    def one_call(leg):
        t0 = time.perf_counter()
        if leg == "torch_callable":
            L.check(core.lbfgsx_trial_point(h, 0.37))
            L.check(core.lbfgsx_sync(h))
            fn(vec(L.VEC_XT), vec(L.VEC_GT))
            torch.cuda.synchronize()
            L.check(core.lbfgsx_trial_dg(h, C.byref(dg)))
        else:
            L.check(core.lbfgsx_trial(h, oid[leg], 0.37, C.byref(fx), C.byref(dg)))
        return (time.perf_counter() - t0) * 1e3

    legs = ["built_in", "chained_rosenbrock", "second_difference", "second_difference_fit", "torch_callable"]
    setup = {"built_in": lambda: L.OBJ_EXT_ROSENBROCK,
             "chained_rosenbrock": lambda: bind(bodies["chained_rosenbrock"]),
             "second_difference": lambda: bind(bodies["second_difference"], scalars=(2.0, 1.0)),
             "second_difference_fit": lambda: bind(bodies["second_difference_fit"], (p0, p1), (2.0,)),
             "torch_callable": lambda: -1}
    oid, times = {}, {k: [] for k in legs}
    for rnd in range(args.rounds):  # round 0 warms every leg up; the legs alternate
        for leg in legs:
            oid[leg] = setup[leg]()
            ms = [one_call(leg) for _ in range(args.calls)]
            if rnd:
                times[leg] += ms[2:]
    med = {k: float(np.median(v)) for k, v in times.items()}
    streams = {"built_in": 4, "chained_rosenbrock": 4, "second_difference": 4, "second_difference_fit": 6}
    rec["trial"] = {"n": n, "dtype": "f64", "step": 0.37, "timed_calls_per_leg": len(times["built_in"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "over_built_in": {k: med[k] / med["built_in"] for k in legs},
                    "streams_of_n_elements": streams,
                    "GB_per_s": {k: streams[k] * n * 8 / med[k] / 1e6 for k in streams},
                    "torch_over_chained_rosenbrock": med["torch_callable"] / med["chained_rosenbrock"]}
    core.lbfgsx_destroy(h)
    del p0, p1
    torch.cuda.empty_cache()

    # ---- cfg4's shape under L-BFGS-B
    nb = args.box_n
    rng = np.random.default_rng(1)
    a = torch.as_tensor(1.0 + 9.0 * rng.random(nb), device="cuda:0")
    b = torch.as_tensor(rng.standard_normal(nb) * 5.0, device="cuda:0")
    box = {"n": nb, "dtype": "f64", "m": 10, "iterations": args.box_iters, "built_in_quadratic": [], "chained_rosenbrock": []}
    sb = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=0.0, epsilon_rel=0.0, past=0, max_iterations=args.box_iters))
    ctx = sb.prepare(nb)
    for which, src in ((L.VEC_A, a), (L.VEC_B, b)):
        L.device_tensor(core.lbfgsx_vec(ctx, which), (nb,), np.float64, 0).copy_(src)
    ones = torch.ones(nb, dtype=torch.float64, device="cuda:0")
    xb = torch.zeros(nb, dtype=torch.float64, device="cuda:0")
    cases = (("built_in_quadratic", A.DiagQuadratic(), -ones, ones), ("chained_rosenbrock", bodies["chained_rosenbrock"], -0.5 * ones, 2.0 * ones))
    for rnd in range(args.rounds):
        for name, f, lb, ub in cases:
            xb.zero_()
            torch.cuda.synchronize()
            ahead0 = (C.c_int64 * 2)()
            core.lbfgsx_b_trial_ahead_counts(sb.ctx, C.byref(ahead0))
            t0 = time.perf_counter()
            niter, fval = sb.minimize(f, xb, lb, ub)
            dt = time.perf_counter() - t0
            ahead = (C.c_int64 * 2)()
            core.lbfgsx_b_trial_ahead_counts(sb.ctx, C.byref(ahead))
            if rnd:
                box[name].append({"s": dt, "niter": niter, "nfev": sb.last.nfev, "fx": fval, "iterations_per_s": niter / dt,
                                  "ms_per_evaluation_of_the_whole_solve": dt * 1e3 / sb.last.nfev,
                                  "first_trials_ahead": ahead[0] - ahead0[0], "taken_over": ahead[1] - ahead0[1]})
    rec["box"] = box
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"median_ms": med, "over_built_in": rec["trial"]["over_built_in"],
                      "box_iterations_per_s": {k: float(np.median([r["iterations_per_s"] for r in box[k]])) for k, *_ in cases}}))


if __name__ == "__main__":
    main()
