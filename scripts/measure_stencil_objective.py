#!/usr/bin/env python3
"""What a grid stencil objective (lbfgspp_amd.StencilObjective) costs, in one process on one device
(profiles/stencil_objective.json).

  trial   10000 x 10000 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around
          the synchronous call, median of 20 timed calls after warm-up, the tile order alternating as in a search; the legs
          alternate, so every ratio is taken inside one process on one device) of the Swift-Hohenberg / plate energy
              sum over the patches of 1/2 (x1 + x3 + x5 + x7 - 4 x4)^2 + c0/4 (x4^2 - 1)^2
          on the open grid and on the torus, against (a) the built-in ExtendedRosenbrock at that n, (b) PeriodicGridObjective
          with the Allen-Cahn cell on the same shape and (c) the torch callable of the same energy (slices on the open grid,
          torch.roll on the torus; trial point + callable + grad.d: what a DeviceObjective costs per evaluation, the only route
          to this energy without the form).
  code    VGPRs and scratch of the compiled bodies, from the code object.

The bytes of one k_stencil_trial launch past L2 are a counter run of their own: rocprofv3 --pmc FETCH_SIZE, then --pmc
WRITE_SIZE, one counter per run and never with tracing, over --pmc-program (a few trial calls of the built-in and of the torus,
nothing written); --counters folds the csv files into the json.

    python scripts/measure_stencil_objective.py [--out profiles/stencil_objective.json] [--grid-side 10000]
    rocprofv3 --pmc FETCH_SIZE -d <dir> -o fetch --output-format csv -- python scripts/measure_stencil_objective.py --pmc-program
    python scripts/measure_stencil_objective.py --counters <dir>/.../fetch_counter_collection.csv <dir>/.../write_counter_collection.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

C0 = 4.0
STEP = 0.37


def plate_torch(torch, shape, torus):
    """the plate energy and its gradient on torch tensors: every patch has the five-point Laplacian at its centre"""
    def fn(x, g):
        X = x.view(shape)
        G = g.view(shape)
        if torus:  # every node is the centre of one patch
            def lap(u):
                return torch.roll(u, 1, 0) + torch.roll(u, -1, 0) + torch.roll(u, 1, 1) + torch.roll(u, -1, 1) - 4.0 * u
            l = lap(X)
            u = X * X - 1.0
            G.copy_(lap(l) + C0 * (u * X))
            return float((0.5 * (l * l) + (0.25 * C0) * (u * u)).sum())
        c = X[1:-1, 1:-1]  # the centres are the interior nodes
        l = X[:-2, 1:-1] + X[2:, 1:-1] + X[1:-1, :-2] + X[1:-1, 2:] - 4.0 * c
        u = c * c - 1.0
        G.zero_()
        G[1:-1, 1:-1] += C0 * (u * c) - 4.0 * l
        G[:-2, 1:-1] += l
        G[2:, 1:-1] += l
        G[1:-1, :-2] += l
        G[1:-1, 2:] += l
        return float((0.5 * (l * l) + (0.25 * C0) * (u * u)).sum())
    return fn


class Bench:
    """one context of n f64 coordinates with random xp and d, ready for trial evaluations"""

    def __init__(self, torch, core, L, n):
        self.torch, self.core, self.L, self.n = torch, core, L, n
        self.h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(self.h), L.F64, n, 1, 0, 0))
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        self.vec(L.VEC_X).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        self.vec(L.VEC_D).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(self.h))
        self.fx, self.dg = C.c_double(), C.c_double()

    def vec(self, v):
        return self.L.device_tensor(self.core.lbfgsx_vec(self.h, v), (self.n,), np.float64, 0)

    def trial(self, oid):
        t0 = time.perf_counter()
        self.L.check(self.core.lbfgsx_trial(self.h, oid, STEP, C.byref(self.fx), C.byref(self.dg)))
        return (time.perf_counter() - t0) * 1e3

    def callable_trial(self, fn):
        t0 = time.perf_counter()
        self.L.check(self.core.lbfgsx_trial_point(self.h, STEP))
        self.L.check(self.core.lbfgsx_sync(self.h))
        self.f_callable = fn(self.vec(self.L.VEC_XT), self.vec(self.L.VEC_GT))
        self.torch.cuda.synchronize()
        self.L.check(self.core.lbfgsx_trial_dg(self.h, C.byref(self.dg)))
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.core.lbfgsx_destroy(self.h)
        self.torch.cuda.empty_cache()


def fold_counters(paths):
    """{kernel: {counter: [value per launch]}} of rocprofv3's counter_collection csv files"""
    out = {}
    for path in paths:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                kernel = "k_stencil_trial" if "k_stencil_trial" in name else "k_trial_built_in" if "k_trial" in name else None
                if kernel:
                    out.setdefault(kernel, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stencil_objective.json"))
    ap.add_argument("--grid-side", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=12, help="per leg and round; the first two of a round are not timed")
    ap.add_argument("--rounds", type=int, default=3, help="round 0 warms up: 2 timed rounds of 10 calls are the 20")
    ap.add_argument("--pmc-program", action="store_true", help="a few trial calls of the built-in and of the torus, no file")
    ap.add_argument("--counters", nargs="+", metavar="CSV", help="fold rocprofv3 counter files into the counters entry of --out")
    args = ap.parse_args()
    shape = (args.grid_side, args.grid_side)
    n = shape[0] * shape[1]
    if args.counters:
        rec = json.load(open(args.out))
        got = fold_counters(args.counters)
        rec["counters"] = {"what": "rocprofv3 --pmc, one counter per run, the torus, f64, beside the built-in at the same n, per "
                                   "launch as reported (see profiles/grid_objective.json on what FETCH_SIZE reports on gfx950)",
                           "model_bytes": {"read": 16 * n, "written": 16 * n}}
        rec["counters"].update(got)
        sten, blt = got.get("k_stencil_trial", {}), got.get("k_trial_built_in", {})
        for name in ("FETCH_SIZE", "WRITE_SIZE"):
            if name in sten and name in blt:
                rec["counters"][name.lower() + "_over_built_in"] = float(np.median(sten[name]) / np.median(blt[name]))
        json.dump(rec, open(args.out, "w"))
        print(json.dumps({k: v for k, v in rec["counters"].items() if k != "what"}))
        return
    import torch

    import lbfgspp_amd as A
    import periodic_ref as PR
    import stencil_ref as SR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_stencil_objective.py needs a GPU")
    cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)
    sten = A.StencilObjective(SR.PLATE, shape=shape, scalars=(C0,))
    pgrid = A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape, scalars=(C0,))
    b = Bench(torch, core, L, n)

    def bind_stencil(mask):
        oid = C.c_int(-1)
        L.check(core.lbfgsx_objective_bind_grid_stencil(b.h, sten.compile(), *shape, mask, None, C.byref(cs), C.byref(oid)))
        return oid.value

    def bind_pgrid():
        oid = C.c_int(-1)
        L.check(core.lbfgsx_objective_bind_grid_periodic(b.h, pgrid.compile(), *shape, 3, None, C.byref(cs), C.byref(oid)))
        return oid.value

    if args.pmc_program:
        for _ in range(2):
            b.trial(L.OBJ_EXT_ROSENBROCK)
        oid = bind_stencil(3)
        for _ in range(4):
            b.trial(oid)
        b.close()
        return

    rec = {"device": torch.cuda.get_device_name(0), "code": {"stencil_plate": sten.info(), "periodic_grid_allen_cahn": pgrid.info()}}
    times, checks = {}, {}
    # the callables against the kernels at one trial point: f of the same energy (a sanity check of the callables)
    for mask, torus in ((0, False), (3, True)):
        b.trial(bind_stencil(mask))
        f_kernel = b.fx.value
        b.callable_trial(plate_torch(torch, shape, torus))
        checks["mask%d" % mask] = {"f_kernel": f_kernel, "f_torch": b.f_callable}
    state = {}

    def leg(key, make):
        def call():
            if state.get("bound") != key:
                state["oid"], state["bound"] = make(), key
            return b.trial(state["oid"])
        return call
    legs = [("built_in", lambda: b.trial(L.OBJ_EXT_ROSENBROCK)),
            ("stencil_open", leg("open", lambda: bind_stencil(0))),
            ("stencil_torus", leg("torus", lambda: bind_stencil(3))),
            ("periodic_grid_torus", leg("pgrid", bind_pgrid)),
            ("torch_open", lambda f=plate_torch(torch, shape, False): b.callable_trial(f)),
            ("torch_torus", lambda f=plate_torch(torch, shape, True): b.callable_trial(f))]
    for name, _ in legs:
        times[name] = []
    for rnd in range(args.rounds):  # round 0 warms every leg up, the legs alternate
        for name, call in legs:
            ms = [call() for _ in range(args.calls)]
            if rnd:
                times[name] += ms[2:]
    b.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec["trial"] = {"shape": list(shape), "n": n, "dtype": "f64", "step": STEP, "c0": C0,
                    "timed_calls_per_leg": len(times["stencil_torus"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "ratios": {"stencil_open_over_built_in": med["stencil_open"] / med["built_in"],
                               "stencil_torus_over_built_in": med["stencil_torus"] / med["built_in"],
                               "stencil_torus_over_periodic_grid": med["stencil_torus"] / med["periodic_grid_torus"],
                               "torch_open_over_stencil_open": med["torch_open"] / med["stencil_open"],
                               "torch_torus_over_stencil_torus": med["torch_torus"] / med["stencil_torus"]},
                    "callable_checks": checks}
    json.dump(rec, open(args.out, "w"))
    print(json.dumps(rec["trial"]))


if __name__ == "__main__":
    main()
