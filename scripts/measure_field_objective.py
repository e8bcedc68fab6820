#!/usr/bin/env python3
"""What a grid field objective (lbfgspp_amd.GridFieldObjective) costs, in one process on one device
(profiles/field_objective.json).

  trial   n ~ 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of the timed calls after warm-up, the tile order alternating as in a search; the legs of a
          context alternate, so every ratio is taken inside one process on one device) of the Ginzburg-Landau energy
            D = 2 on 7071 x 7071 and D = 3 on 5773 x 5774, open (mask 0) and on the torus (mask 3), against
              (1) the built-in ExtendedRosenbrock at that n,
              (3) MeshObjective with K = 4 and the same D on the quad mesh of the same lattice (mask 0),
              (4) a torch callable of the same energy (trial point + callable + grad.d: what a DeviceObjective costs per
                  evaluation), written with slices for the open grid and with torch.roll for the torus;
            (2) PeriodicGridObjective Allen-Cahn on 10000 x 10000, with the built-in at that n, in a context of its own.
          Reported: the medians, ms per 1e8 coordinates against (2), and the ratios to (3) and (4).
  code    VGPRs and scratch of the compiled bodies, from the code object.

The bytes of one k_gfield_trial launch past L2 are a counter run of their own: rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE,
no tracing combined, around this script with --pmc-program D, which makes a few lbfgsx_trial calls of the built-in and of the
torus at that D; --counters folds the csv files into the json beside the byte model (xp and d read, x and grad written):

    python scripts/measure_field_objective.py [--out profiles/field_objective.json]
    rocprofv3 --pmc FETCH_SIZE -d <dir> -o fetch --output-format csv -- python scripts/measure_field_objective.py --pmc-program 2
    python scripts/measure_field_objective.py --counters <dir>/*counter_collection.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

C0 = 4.0
STEP = 0.37
SHAPES = {2: (7071, 7071), 3: (5773, 5774)}


def gl_torch(torch, shape, D, torus):
    """the Ginzburg-Landau energy and its gradient: every lattice edge inside the grid has the weight 1/2 in total (two cells,
    a quarter each), an edge on an open side the weight 1/4 (one cell); the well term at the nodes that start a cell"""
    full = tuple(shape) + (D,)

    def fn(x, g):
        X = x.view(full)
        G = g.view(full)
        u = (X * X).sum(dim=2, keepdim=True) - 1.0
        if torus:
            G.copy_(C0 * (u * X))
            e = float(((0.25 * C0) * (u * u)).sum())
            for ax in (0, 1):
                d = torch.roll(X, -1, ax) - X
                e += float((0.5 * (d * d)).sum())
                G.sub_(d)
                G.add_(torch.roll(d, 1, ax))
            return e
        uc = u[:-1, :-1]
        G.zero_()
        G[:-1, :-1].add_(C0 * (uc * X[:-1, :-1]))
        e = float(((0.25 * C0) * (uc * uc)).sum())
        for ax in (0, 1):
            d = X[1:, :] - X[:-1, :] if ax == 0 else X[:, 1:] - X[:, :-1]
            # the edge's cells: those on either side of it, fewer on the open sides
            w = torch.full(d.shape[:2] + (1,), 0.5, dtype=X.dtype, device=X.device)
            if ax == 0:
                w[:, 0] = 0.25
                w[:, -1] = 0.25
            else:
                w[0, :] = 0.25
                w[-1, :] = 0.25
            wd = w * d
            e += float((wd * d).sum())
            wd = 2.0 * wd
            if ax == 0:
                G[1:, :].add_(wd)
                G[:-1, :].sub_(wd)
            else:
                G[:, 1:].add_(wd)
                G[:, :-1].sub_(wd)
        return e
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


def quad_mesh(shape):
    rows, cols = shape
    origin = (np.arange(rows - 1, dtype=np.int64)[:, None] * cols + np.arange(cols - 1, dtype=np.int64)[None, :]).reshape(-1)
    return np.ascontiguousarray(np.stack([origin, origin + 1, origin + cols, origin + cols + 1], 1), np.int32)


def fold_counters(paths):
    """{kernel: {counter: [value per launch]}} of rocprofv3's counter_collection csv files"""
    out = {}
    for path in paths:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                kernel = "k_gfield_trial" if "k_gfield_trial" in name else "k_trial_built_in" if "k_trial" in name else None
                if kernel:
                    out.setdefault(kernel, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_objective.json"))
    ap.add_argument("--grid-side", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pmc-program", type=int, metavar="D", help="a few trial calls of the built-in and of the torus at D, no file")
    ap.add_argument("--counters", nargs="+", metavar="CSV", help="fold rocprofv3 counter files into the counters entry of --out")
    args = ap.parse_args()
    if args.counters:
        rec = json.load(open(args.out))
        got = fold_counters(args.counters)
        D = rec.get("counters_D", 2)
        n = SHAPES[D][0] * SHAPES[D][1] * D
        rec["counters"] = {"what": "rocprofv3 --pmc, one counter per run, the torus at D = %d, f64, beside the built-in at the same "
                                   "n, per launch as reported (see profiles/grid_objective.json on what FETCH_SIZE reports on gfx950)" % D,
                           "model_bytes": {"read": 16 * n, "written": 16 * n}}
        rec["counters"].update(got)
        fld, blt = got.get("k_gfield_trial", {}), got.get("k_trial_built_in", {})
        for name in ("FETCH_SIZE", "WRITE_SIZE"):
            if name in fld and name in blt:
                rec["counters"][name.lower() + "_over_built_in"] = float(np.median(fld[name]) / np.median(blt[name]))
        json.dump(rec, open(args.out, "w"))
        print(json.dumps({k: v for k, v in rec["counters"].items() if k != "what"}))
        return
    import torch

    import field_ref as FR
    import lbfgspp_amd as A
    import periodic_ref as PR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_field_objective.py needs a GPU")
    cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)
    field = {D: A.GridFieldObjective(FR.GL, shape=SHAPES[D], D=D, scalars=(C0,)) for D in SHAPES}

    def bind_field(b, D, mask):
        oid = C.c_int(-1)
        L.check(core.lbfgsx_objective_bind_grid_field(b.h, field[D].compile(), *SHAPES[D], mask, None, C.byref(cs), C.byref(oid)))
        return oid.value

    if args.pmc_program:
        D = args.pmc_program
        b = Bench(torch, core, L, SHAPES[D][0] * SHAPES[D][1] * D)
        for _ in range(2):
            b.trial(L.OBJ_EXT_ROSENBROCK)
        oid = bind_field(b, D, 3)
        for _ in range(4):
            b.trial(oid)
        b.close()
        return

    gshape = (args.grid_side, args.grid_side)
    pgrid = A.PeriodicGridObjective(PR.ALLENCAHN, shape=gshape, scalars=(C0,))
    rec = {"device": torch.cuda.get_device_name(0), "code": {"periodic_grid_allen_cahn": pgrid.info()}}
    times, checks = {}, {}

    def run(legs):
        """legs: [(name, call)]; round 0 warms every leg up, the legs of a context alternate"""
        for name, _ in legs:
            times[name] = []
        for rnd in range(args.rounds):
            for name, call in legs:
                ms = [call() for _ in range(args.calls)]
                if rnd:
                    times[name] += ms[2:]

    for D, shape in SHAPES.items():
        n = shape[0] * shape[1] * D
        # the element body: the mesh form names the element's nodes v, the cell's text has a local of that name
        mesh = A.MeshObjective(re.sub(r"\bv\b", "val", FR.GL), quad_mesh(shape), D, scalars=(C0,))
        rec["code"]["field_D%d" % D] = field[D].info()
        rec["code"]["mesh_D%d" % D] = mesh.info()
        b = Bench(torch, core, L, n)
        el = mesh.elements

        def bind_mesh():
            oid = C.c_int(-1)
            L.check(core.lbfgsx_objective_bind_mesh(b.h, mesh.compile(), el.shape[0], el.ctypes.data_as(C.c_void_p), 0, None,
                                                    C.byref(cs), C.byref(oid)))
            return oid.value

        # the callables against the kernels at one trial point: f of the same energy (a sanity check of the callables)
        for mask, torus in ((0, False), (3, True)):
            b.trial(bind_field(b, D, mask))
            f_kernel = b.fx.value
            b.callable_trial(gl_torch(torch, shape, D, torus))
            checks["D%d_mask%d" % (D, mask)] = {"f_kernel": f_kernel, "f_torch": b.f_callable}
        state = {}

        def leg(key, make):
            def call():
                if state.get("bound") != key:
                    state["oid"], state["bound"] = make(), key
                return b.trial(state["oid"])
            return call
        run([("built_in_D%d" % D, lambda: b.trial(L.OBJ_EXT_ROSENBROCK)),
             ("field_open_D%d" % D, leg("open", lambda: bind_field(b, D, 0))),
             ("field_torus_D%d" % D, leg("torus", lambda: bind_field(b, D, 3))),
             ("mesh_open_D%d" % D, leg("mesh", bind_mesh)),
             ("torch_open_D%d" % D, lambda f=gl_torch(torch, shape, D, False): b.callable_trial(f)),
             ("torch_torus_D%d" % D, lambda f=gl_torch(torch, shape, D, True): b.callable_trial(f))])
        b.close()
        del mesh, el
    b = Bench(torch, core, L, gshape[0] * gshape[1])
    oid = C.c_int(-1)
    L.check(core.lbfgsx_objective_bind_grid_periodic(b.h, pgrid.compile(), *gshape, 3, None, C.byref(cs), C.byref(oid)))
    run([("built_in_at_grid_n", lambda: b.trial(L.OBJ_EXT_ROSENBROCK)), ("periodic_grid_torus", lambda: b.trial(oid.value))])
    b.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    per = {}
    for D, shape in SHAPES.items():
        n = shape[0] * shape[1] * D
        for mask in ("open", "torus"):
            ms = med["field_%s_D%d" % (mask, D)]
            per["field_%s_D%d" % (mask, D)] = {
                "ms_per_1e8": ms * 1e8 / n,
                "over_periodic_grid_per_coordinate": (ms * 1e8 / n) / (med["periodic_grid_torus"] * 1e8 / (gshape[0] * gshape[1])),
                "over_built_in": ms / med["built_in_D%d" % D],
                "torch_over_field": med["torch_%s_D%d" % (mask, D)] / ms}
        per["field_open_D%d" % D]["mesh_over_field"] = med["mesh_open_D%d" % D] / med["field_open_D%d" % D]
    rec["trial"] = {"shapes": {"D%d" % D: list(s) for D, s in SHAPES.items()}, "periodic_grid_shape": list(gshape),
                    "n": {"D%d" % D: s[0] * s[1] * D for D, s in SHAPES.items()}, "dtype": "f64", "step": STEP, "c0": C0,
                    "timed_calls_per_leg": len(times["periodic_grid_torus"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()}, "ratios": per, "callable_checks": checks}
    json.dump(rec, open(args.out, "w"))
    print(json.dumps(rec["trial"]))


if __name__ == "__main__":
    main()
