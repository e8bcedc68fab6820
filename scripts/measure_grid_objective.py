#!/usr/bin/env python3
"""What a grid objective (2x2-cell terms on a row-major grid, lbfgspp_amd.GridObjective) costs, in one process on one device
(profiles/grid_objective.json).

  trial   n = 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of the timed calls after warm-up, the tile order alternating as in a search) for
          (a) the built-in ExtendedRosenbrock, (b) the K = 2 chained Rosenbrock, (c) the Allen-Cahn energy on 10000 x 10000
          (cols % W == 0: the rows above and below are 16-byte loads), (d) the same on 9999 x 10001 (element loads) and
          (e) the torch callable of (c) (trial point + callable + grad.d, what a DeviceObjective costs per evaluation).
          The yardsticks of (c) are (a) and (b) of the same run: the byte model is the same four streams.
  box     cfg4's shape as a grid (3162 x 3162 f64, m = 10) under L-BFGS-B: the Allen-Cahn energy in the box [-0.5, 0.9] beside
          the built-in quadratic in [-1, 1]; iterations per second and how many first trials rode on the dg / max-step pass.
  code    VGPRs and scratch of the compiled bodies, from the code object.

The bytes of one k_grid_trial launch past L2 are a counter run of their own (rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE,
no tracing combined, around a program that makes a few lbfgsx_trial calls); its figures are the "counters" entry of the file.

    python scripts/measure_grid_objective.py [--out profiles/grid_objective.json] [--rows 10000] [--cols 10000]
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
ALLENCAHN = """const T a = x[1] - x[0];
const T b = x[2] - x[0];
const T e = x[3] - x[2];
const T h = x[3] - x[1];
const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[0]);
g[1] = T(0.5) * (a - h);
g[2] = T(0.5) * (b - e);
g[3] = T(0.5) * (e + h);
return T(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u);"""
C0 = 4.0


def allencahn_torch(torch, rows, cols):
    def fn(x, g):
        X = x.view(rows, cols)
        G = g.view(rows, cols)
        x0, x1, x2, x3 = X[:-1, :-1], X[:-1, 1:], X[1:, :-1], X[1:, 1:]
        a, b, e, h = x1 - x0, x2 - x0, x3 - x2, x3 - x1
        u = x0 * x0 - 1.0
        g.zero_()
        G[:-1, :-1] += -0.5 * (a + b) + C0 * (u * x0)
        G[:-1, 1:] += 0.5 * (a - h)
        G[1:, :-1] += 0.5 * (b - e)
        G[1:, 1:] += 0.5 * (e + h)
        return float((0.25 * ((a * a + b * b) + (e * e + h * h)) + (0.25 * C0) * (u * u)).sum())
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_objective.json"))
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--box-side", type=int, default=3162)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--box-iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_grid_objective.py needs a GPU")
    rec = {"device": torch.cuda.get_device_name(0)}
    chain = A.ChainObjective(CHAINED_ROSEN, K=2)
    grid = A.GridObjective(ALLENCAHN, shape=(args.rows, args.cols), scalars=(C0,))
    rec["code"] = {"chained_rosenbrock": chain.info(), "allen_cahn": grid.info()}

    # ---- one trial evaluation: a context per shape, the legs of a shape alternating
    shapes = {"aligned": (args.rows, args.cols), "unaligned": (args.rows - 1, args.cols + 1)}
    legs_of = {"aligned": ["built_in", "chained_rosenbrock", "allen_cahn_aligned", "torch_callable"],
               "unaligned": ["allen_cahn_unaligned"]}
    times = {}
    for which, (rows, cols) in shapes.items():
        n = rows * cols
        assert which != "aligned" or n % 2 == 0, "the built-in extended Rosenbrock leg needs an even n"
        h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))

        def vec(v):
            return L.device_tensor(core.lbfgsx_vec(h, v), (n,), np.float64, 0)

        gen = torch.Generator(device="cuda:0").manual_seed(1)
        vec(L.VEC_X).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        vec(L.VEC_D).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(h))
        fx, dg = C.c_double(), C.c_double()
        cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)
        fn = allencahn_torch(torch, rows, cols)

        def setup(leg):
            oid = C.c_int(-1)
            if leg == "built_in":
                return L.OBJ_EXT_ROSENBROCK
            if leg == "chained_rosenbrock":
                L.check(core.lbfgsx_objective_bind(h, chain.compile(), None, None, C.byref(oid)))
            elif leg.startswith("allen_cahn"):
                L.check(core.lbfgsx_objective_bind_grid(h, grid.compile(), rows, cols, None, C.byref(cs), C.byref(oid)))
            return oid.value

        def one_call(leg, oid):
            t0 = time.perf_counter()
            if leg == "torch_callable":
                L.check(core.lbfgsx_trial_point(h, 0.37))
                L.check(core.lbfgsx_sync(h))
                fn(vec(L.VEC_XT), vec(L.VEC_GT))
                torch.cuda.synchronize()
                L.check(core.lbfgsx_trial_dg(h, C.byref(dg)))
            else:
                L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
            return (time.perf_counter() - t0) * 1e3

        for leg in legs_of[which]:
            times[leg] = []
        for rnd in range(args.rounds):  # round 0 warms every leg up
            for leg in legs_of[which]:
                oid = setup(leg)
                ms = [one_call(leg, oid) for _ in range(args.calls)]
                if rnd:
                    times[leg] += ms[2:]
        core.lbfgsx_destroy(h)
        torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec["trial"] = {"shapes": {k: list(v) for k, v in shapes.items()}, "dtype": "f64", "step": 0.37,
                    "timed_calls_per_leg": len(times["built_in"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "over_built_in": {k: med[k] / med["built_in"] for k in med},
                    "over_chained_rosenbrock": {k: med[k] / med["chained_rosenbrock"] for k in med},
                    "model_streams_of_n_elements": 4}

    # ---- cfg4's shape under L-BFGS-B
    side = args.box_side
    nb = side * side
    rng = np.random.default_rng(1)
    a = torch.as_tensor(1.0 + 9.0 * rng.random(nb), device="cuda:0")
    b = torch.as_tensor(rng.standard_normal(nb) * 5.0, device="cuda:0")
    box = {"shape": [side, side], "dtype": "f64", "m": 10, "iterations": args.box_iters, "built_in_quadratic": [], "allen_cahn": []}
    sb = A.LBFGSBSolver(A.LBFGSBParam(m=10, epsilon=0.0, epsilon_rel=0.0, past=0, max_iterations=args.box_iters))
    ctx = sb.prepare(nb)
    for which, src in ((L.VEC_A, a), (L.VEC_B, b)):
        L.device_tensor(core.lbfgsx_vec(ctx, which), (nb,), np.float64, 0).copy_(src)
    ones = torch.ones(nb, dtype=torch.float64, device="cuda:0")
    xb = torch.zeros(nb, dtype=torch.float64, device="cuda:0")
    gbox = A.GridObjective(ALLENCAHN, shape=(side, side), scalars=(C0,))
    cases = (("built_in_quadratic", A.DiagQuadratic(), -ones, ones, 0.0), ("allen_cahn", gbox, -0.5 * ones, 0.9 * ones, 0.2))
    for rnd in range(args.rounds):
        for name, f, lb, ub, x0 in cases:
            xb.fill_(x0)
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
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"median_ms": med, "over_built_in": rec["trial"]["over_built_in"],
                      "box_iterations_per_s": {k: float(np.median([r["iterations_per_s"] for r in box[k]])) for k, *_ in cases}}))


if __name__ == "__main__":
    main()
